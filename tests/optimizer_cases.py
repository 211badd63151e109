"""Shared by tests/test_optimizer_cpu.py and tests/test_optimizer_gpu.py: the fixture the reference's own optimizer lines
left (tests/golden/optimizer_cases.npz, made by tests/golden/make_optimizer_golden.py), the tensors and gradients it was
run on (name-seeded, so the file does not store them) and the bound a trajectory is held to.  Nothing here needs a GPU."""
import os

import numpy as np
import torch
from torch import nn

from salience_detr_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("param", "exp_avg", "exp_avg_sq")


def ulp32(x: float) -> float:
    """Spacing of float32 at magnitude ``x``."""
    return float(np.spacing(np.float32(abs(x))))


class Fixture:
    def __init__(self):
        self.d = d = np.load(os.path.join(GOLDEN, "optimizer_cases.npz"))
        self.shapes = [tuple(int(v) for v in s.split(";")) for s in d["shapes"].tolist()]
        self.group_of = d["group_of"].tolist()
        self.grad_scale, self.step_scale = d["grad_scale"], d["step_scale"]
        self.lrs = d["lrs"]
        self.steps = self.lrs.shape[0]
        self.max_norm = float(d["max_norm"])
        self.none_grad = tuple(int(v) for v in d["none_grad"])
        self.zero_grad = tuple(int(v) for v in d["zero_grad"])
        self.strides = d["strides"].tolist()

    def params(self, device="cpu"):
        return [nn.Parameter((syn.det_randn(f"opt.p.{i}", s) * 3).to(device)) for i, s in enumerate(self.shapes)]

    def gradient(self, k, i, device="cpu"):
        if (k, i) == self.none_grad:
            return None
        if (k, i) == self.zero_grad:
            return torch.zeros(self.shapes[i], device=device)
        return (syn.det_randn(f"opt.g.{k}.{i}", self.shapes[i])
                * (float(self.grad_scale[i]) * float(self.step_scale[k]))).to(device)

    def groups(self, params):
        d = self.d
        return [{"params": [p for p, g in zip(params, self.group_of) if g == gi], "lr": float(lr), "weight_decay": float(wd)}
                for gi, (lr, wd) in enumerate(zip(d["group_lr"], d["group_weight_decay"]))]

    def schedulers(self, opt):
        """The fixture's LinearLR + MultiStepLR pair and the function that advances them after step k."""
        warm = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0 / 1000, total_iters=2)
        decay = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1)

        def advance(k):
            if k < 3:
                warm.step()
            if k % 3 == 2:
                decay.step()
        return advance

    def expected(self, kind, k, i):
        return self.d[f"{kind}.{k}.{i}"]

    def check_step(self, k, tensors, norm, d_ref=None, d_ref_norm=None, worst=None):
        """``tensors[i] = (param, exp_avg, exp_avg_sq)`` after step k (k = 0 is the first) against the float64 run:
        every stored element within max(4 * d_ref, (k + 1) * ulp32(max|tensor|)); the norm's relative distance within
        max(4 * d_ref_norm, 2^-22).  ``d_ref`` defaults to the fixture's (the reference's own fp32 distance).  Returns the
        worst error / bound ratio seen (also kept in ``worst`` when given)."""
        d_ref = self.d["d_ref"] if d_ref is None else d_ref
        d_ref_norm = self.d["d_ref_norm"] if d_ref_norm is None else d_ref_norm
        ratios = []
        for i, triple in enumerate(tensors):
            for j, kind in enumerate(KINDS):
                want = self.expected(kind, k, i)
                got = triple[j].detach().double().cpu().reshape(-1)[::self.strides[i]].numpy()
                err = float(np.abs(got - want).max())
                bound = max(4.0 * float(d_ref[k, i, j]), (k + 1) * ulp32(float(np.abs(want).max())))
                ratios.append(err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
                assert err <= bound, (k, i, kind, err, bound, float(d_ref[k, i, j]))
        want = float(self.d["norms"][k])
        rel = abs(float(norm) - want) / want
        bound = max(4.0 * float(d_ref_norm[k]), 2.0 ** -22)
        assert rel <= bound, (k, "norm", rel, bound)
        out = (max(ratios), rel / bound)
        if worst is not None:
            worst.append(out)
        return out

    def distances(self, k, tensors, norm):
        """max |tensor - float64 run| per (tensor, kind) of step k and the norm's relative distance: another run's own
        ``d_ref``."""
        out = np.zeros((len(tensors), 3))
        for i, triple in enumerate(tensors):
            for j, kind in enumerate(KINDS):
                got = triple[j].detach().double().cpu().reshape(-1)[::self.strides[i]].numpy()
                out[i, j] = np.abs(got - self.expected(kind, k, i)).max()
        want = float(self.d["norms"][k])
        return out, abs(float(norm) - want) / want


def state_triples(opt, params):
    """(param, exp_avg, exp_avg_sq) per parameter from an optimizer's ``state`` (zeros before a parameter's first step)."""
    if hasattr(opt, "_sync_state"):
        opt._sync_state()
    out = []
    for p in params:
        s = opt.state.get(p, {})
        out.append((p, s.get("exp_avg", torch.zeros_like(p)), s.get("exp_avg_sq", torch.zeros_like(p))))
    return out


def module_tree(names, norm_names=()):
    """A module tree that registers one small parameter per dotted name, in order; the leaf modules that own a name of
    ``norm_names`` are ``nn.LayerNorm``s (their ``weight`` / ``bias``), all other owners plain modules."""
    root = nn.Module()
    norm_owners = {n.rsplit(".", 1)[0] for n in norm_names}
    for name in names:
        parts = name.split(".")
        node, path = root, []
        for part in parts[:-1]:
            path.append(part)
            if part not in node._modules:
                owner = ".".join(path)
                node.add_module(part, nn.LayerNorm(2) if owner in norm_owners else nn.Module())
            node = node._modules[part]
        if parts[-1] not in node._parameters:
            node.register_parameter(parts[-1], nn.Parameter(torch.zeros(2)))
    assert [n for n, _ in root.named_parameters()] == list(names)
    return root
