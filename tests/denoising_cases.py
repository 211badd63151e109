"""Shared by tests/test_denoising_cpu.py and tests/test_denoising_gpu.py: the fixture's cases
(tests/golden/denoising_cases.npz, made by tests/golden/make_denoising_golden.py from the imported reference) and a
pure-torch restatement of the generator on the kernel's noise tensor -- pinned to the fixture on the CPU, and then the
oracle for shapes the fixture does not hold."""
import os

import numpy as np
import torch

from salience_detr_amd import denoising as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoising_cases.npz")
BOX_BAR = 1e-3      # the project's fp32 parity bar (README: "Parity <= 1e-3 (fp32) against golden vectors")


class Case:
    def __init__(self, data, tag):
        g = lambda k: data[f"{tag}_{k}"] if f"{tag}_{k}" in data else None
        self.tag = tag
        self.counts = [int(c) for c in g("counts")]
        self.C, self.E, self.Nq, self.nums, self.groups, self.twice_max_gt = [int(v) for v in g("params")]
        self.p_label, self.s_box = [float(v) for v in g("noise_params")]
        self.weight = torch.from_numpy(g("weight"))
        self.tboxes = torch.from_numpy(g("tboxes")).reshape(-1, 4)
        self.tlabels = torch.from_numpy(g("tlabels"))
        t = lambda a: None if a is None else torch.from_numpy(a)
        self.flip, self.new_label = t(g("draw_flip")), t(g("draw_label"))
        self.sign, self.magnitude = t(g("draw_sign")), t(g("draw_magnitude"))
        self.noised_labels = torch.from_numpy(g("noised_labels"))
        self.box_queries = torch.from_numpy(g("box_queries"))
        self.label_queries = t(g("label_queries"))
        side = int(g("mask_side")[0])
        self.mask = torch.from_numpy(np.unpackbits(g("mask_bits"))[:side * side].reshape(side, side).astype(bool))
        self.max_gt = max(self.counts)
        self.n_dn = 2 * self.groups * self.max_gt

    def targets(self):
        out, o = [], 0
        for n in self.counts:
            out.append({"boxes": self.tboxes[o:o + n].clone(), "labels": self.tlabels[o:o + n].long()})
            o += n
        return out

    def noise(self, capacity=None):
        cap = max(self.max_gt, 1) if capacity is None else capacity
        return D.pack_noise(self.counts, self.groups, self.C, cap, self.flip, self.new_label, self.sign, self.magnitude)

    def expected_label_queries(self):
        """``weight[noised_labels]`` with zero rows on padding: what the fixture's generator checked bit for bit."""
        out = torch.zeros(len(self.counts), self.n_dn, self.E)
        ok = self.noised_labels >= 0
        out[ok] = self.weight[self.noised_labels[ok].long()]
        return out


def load_cases():
    data = np.load(GOLDEN)
    return {str(tag): Case(data, str(tag)) for tag in data["tags"]}


def inverse_sigmoid(x, eps=1e-3):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def restate(counts, tboxes, tlabels, weight, noise, max_gt, groups, num_queries, p_label, s_box, capacity):
    """The generator in plain torch on the kernel's inputs (staged layout: image b's targets packed from
    ``sum(counts[:b])``; noise ``[2 * groups, B * capacity, 10]``).  Returns ``(label_queries, box_queries, noised_labels,
    attn_mask)``; fp32 throughout, the reference's operation order."""
    B, (C, E) = len(counts), weight.shape
    n_dn = 2 * groups * max_gt
    label_q = torch.zeros(B, n_dn, E)
    box_q = torch.zeros(B, n_dn, 4)
    noised = torch.full((B, n_dn), -1, dtype=torch.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    for b, n in enumerate(counts):
        if n == 0:
            continue
        rows = torch.arange(offsets[b], offsets[b] + n)
        for r in range(2 * groups):
            u = noise[r, rows].float()
            labels = tlabels[rows].long()
            if p_label > 0:
                new = torch.clamp((u[:, 1] * C).floor().long(), max=C - 1)
                labels = torch.where(u[:, 0] < torch.tensor(p_label * 0.5, dtype=torch.float32), new, labels)
            boxes = tboxes[rows].float().clone()
            if s_box > 0:
                half = boxes[:, 2:] / 2
                diff = torch.cat([half, half], -1)
                sign = (u[:, 2:6] >= 0.5).float() * 2.0 - 1.0
                part = u[:, 6:10].clone()
                if r % 2 == 1:
                    part = part + 1.0
                part = part * sign
                cx, cy, w, h = boxes.unbind(-1)
                xyxy = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), -1)
                xyxy = (xyxy + (part * diff) * s_box).clamp(0.0, 1.0)
                x1, y1, x2, y2 = xyxy.unbind(-1)
                boxes = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), -1)
            sl = slice(r * max_gt, r * max_gt + n)
            label_q[b, sl] = weight[labels]
            box_q[b, sl] = inverse_sigmoid(boxes)
            noised[b, sl] = labels.int()
    return label_q, box_q, noised, D.query_mask(max_gt, groups, num_queries)


def restate_case(case, capacity=None):
    cap = max(case.max_gt, 1) if capacity is None else capacity
    return restate(case.counts, case.tboxes, case.tlabels, case.weight, case.noise(cap), case.max_gt, case.groups, case.Nq,
                   case.p_label, case.s_box, cap)


def random_targets(counts, C, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in counts:
        cxcy = torch.rand(n, 2, generator=g) * 0.8 + 0.1
        wh = torch.rand(n, 2, generator=g) * 0.5 + 0.02
        out.append({"boxes": torch.cat([cxcy, wh], -1), "labels": torch.randint(0, C, (n,), generator=g)})
    return out
