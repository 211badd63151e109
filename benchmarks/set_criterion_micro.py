"""Micro-benchmark of the set criterion (row N6): match + loss forward + backward of every output of a step at B = 2,
Nq = 900, C = 91, 6 decoder outputs + the encoder output, T targets per image in {7, 20, 100}.

Compared with the torch composite of the reference's HybridSetCriterion on the device: the cost in torch ops, the
assignment by scipy's linear_sum_assignment on the host (when scipy is installed; otherwise by this library's assignment
kernel, named in the output), the losses in torch ops with autograd.  Times are device-event / synchronised host-clock
medians; launch counts are kernel records of torch.profiler.  Prints one JSON line per T.

    python benchmarks/set_criterion_micro.py [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from salience_detr_amd import set_criterion as S  # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment
except ImportError:  # the GPU machine may not have scipy
    linear_sum_assignment = None

DEV = "cuda:0"
B, NQ, C, NOUT = 2, 900, 91, 7


def inputs(T, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(NOUT, B, NQ, C, generator=g) * 1.5 - 3.0
    boxes = torch.cat([torch.rand(NOUT, B, NQ, 2, generator=g) * 0.8 + 0.1,
                       torch.rand(NOUT, B, NQ, 2, generator=g) * 0.3 + 0.02], -1)
    targets = [{"boxes": torch.cat([torch.rand(T, 2, generator=g) * 0.8 + 0.1, torch.rand(T, 2, generator=g) * 0.3 + 0.02],
                                   -1).to(DEV), "labels": torch.randint(0, C, (T,), generator=g).to(DEV)} for _ in range(B)]
    return logits.to(DEV).requires_grad_(True), boxes.to(DEV).requires_grad_(True), targets


def outputs_of(lg, bx):
    return {"pred_logits": lg[0], "pred_boxes": bx[0],
            "aux_outputs": [{"pred_logits": lg[i], "pred_boxes": bx[i]} for i in range(1, NOUT - 1)],
            "enc_outputs": {"pred_logits": lg[NOUT - 1], "pred_boxes": bx[NOUT - 1]}}


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_pairs(a, b):
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    ewh = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area_c = ewh[..., 0] * ewh[..., 1]
    iou = inter / union
    return iou, iou - (area_c - union) / area_c


def composite(lg, bx, targets, staged):
    """The reference's criterion as torch ops (matching by scipy on the host, or by this library's kernel)."""
    nb = max(sum(len(t["labels"]) for t in targets), 1)
    total = 0.0
    for o in range(NOUT):
        if linear_sum_assignment is not None:
            idx = []
            with torch.no_grad():
                for b, t in enumerate(targets):
                    p = lg[o, b].sigmoid()
                    neg = -0.75 * p ** 2 * (1 - p + 1e-6).log()
                    pos = -0.25 * (1 - p) ** 2 * (p + 1e-6).log()
                    cls = pos[:, t["labels"]] - neg[:, t["labels"]]
                    l1 = torch.cdist(bx[o, b], t["boxes"], p=1)
                    _, g = giou_pairs(xyxy(bx[o, b])[:, None], xyxy(t["boxes"])[None])
                    c = 5 * l1 + 2 * cls - 2 * g
                    r, k = linear_sum_assignment(c.cpu())
                    idx.append((torch.as_tensor(r, device=DEV), torch.as_tensor(k, device=DEV)))
        else:
            m = S.match_outputs([lg[o]], [bx[o]], staged, 2, 5, 2, 0.25, 2.0)[0]
            idx = [(torch.nonzero(m[b] >= 0).flatten(), m[b][m[b] >= 0].long()) for b in range(B)]
        bi = torch.cat([torch.full_like(s, b) for b, (s, _) in enumerate(idx)])
        si = torch.cat([s for s, _ in idx])
        src = bx[o][bi, si]
        tgt = torch.cat([t["boxes"][k] for t, (_, k) in zip(targets, idx)])
        iou, giou = giou_pairs(xyxy(src), xyxy(tgt))
        labels = torch.cat([t["labels"][k] for t, (_, k) in zip(targets, idx)])
        onehot = torch.zeros_like(lg[o])
        onehot[bi, si, labels] = 1
        score = torch.zeros_like(lg[o])
        score[bi, si, labels] = iou.detach()
        prob = lg[o].sigmoid().detach()
        w = 0.75 * prob ** 2 * (1 - onehot) + score
        cls = torch.nn.functional.binary_cross_entropy_with_logits(lg[o], score, weight=w, reduction="sum") / nb
        total = total + cls + 5 * (src - tgt).abs().sum() / nb + 2 * (1 - giou).sum() / nb
    return total


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    times.sort()
    return times[len(times) // 2]


def event_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3)
    res.sort()
    return res[len(res) // 2]


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    crit = S.HybridSetCriterion(C, S.HungarianMatcher(2, 5, 2), {})
    for T in (7, 20, 100):
        lg, bx, targets = inputs(T, seed=T)
        staged = S.stage_targets(targets, capacity=T)
        outs = [lg[i] for i in range(NOUT)], [bx[i] for i in range(NOUT)]
        holder = {}

        def match():
            holder["m"] = crit.matcher.match(*outs, staged, [False] * NOUT)[0]

        def fwd():
            holder["L"] = S.set_losses(*outs, staged, holder["m"])

        def bwd():
            torch.autograd.grad(holder["L"].sum(), [lg, bx])

        def whole():
            losses = crit(outputs_of(lg, bx), None, staged=staged)
            torch.autograd.grad(torch.stack(list(losses.values())).sum(), [lg, bx])

        def comp():
            torch.autograd.grad(composite(lg, bx, targets, staged), [lg, bx])

        match()
        fwd()
        rec = {"T": T, "B": B, "Nq": NQ, "C": C, "outputs": NOUT,
               "match_us": round(event_us(match, args.iters), 1), "loss_fwd_us": round(event_us(fwd, args.iters), 1),
               "loss_bwd_us": round(event_us(lambda: (fwd(), bwd()), args.iters) - event_us(fwd, args.iters), 1),
               "criterion_us": round(timed(whole, args.iters), 1), "criterion_launches": kernel_launches(whole),
               "composite_matching": "scipy" if linear_sum_assignment is not None else "hip_kernel",
               "composite_us": round(timed(comp, max(3, args.iters // 4)), 1), "composite_launches": kernel_launches(comp)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
