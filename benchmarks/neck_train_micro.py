"""Training the RepVGGPluX neck (row N3): one forward + backward of ``forward_levels`` in ``train()`` mode, the ``"hip"``
form (csrc/neck_backward.hip) against the ``"torch"`` composite on the same device.

The workload: B = 2, C = 256, groups 4, four token-major fp32 levels 100 x 167, 50 x 84, 25 x 42, 13 x 21; every level and
every parameter requires grad, fixed cotangents.  Prints one JSON line:
  hip_us / torch_us            forward + backward, HIP events around it, the median of --iters after --warmup
  hip_forward_us / torch_forward_us   the forward alone (under autograd: what is stored is stored)
  hip_over_torch               hip_us / torch_us
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402
from salience_detr_amd.salience_neck import build_neck  # noqa: E402

SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2)
    args = ap.parse_args()
    m = build_neck(256, len(SHAPES), 4)
    m.load_state_dict(syn.det_state_dict(m.state_dict()))
    m = m.cuda().train()
    levels = [syn.det_randn(f"neck_train_micro.x{l}", (args.batch, h * w, 256)).cuda().requires_grad_(True)
              for l, (h, w) in enumerate(SHAPES)]
    cots = [(syn.det_rand(f"neck_train_micro.g{l}", tuple(x.shape)) - 0.5).cuda() for l, x in enumerate(levels)]

    def forward():
        return m.forward_levels(levels, SHAPES)

    def step():
        m.zero_grad(set_to_none=True)
        for x in levels:
            x.grad = None
        torch.autograd.backward(forward(), cots)

    res = {"batch": args.batch, "channels": 256, "levels": SHAPES, "iters": args.iters}
    for form in ("torch", "hip"):
        m.set_train_form(form)
        res[f"{form}_us"] = timed(step, args.warmup, args.iters)
        res[f"{form}_forward_us"] = timed(forward, args.warmup, args.iters)
    res["hip_over_torch"] = res["hip_us"] / res["torch_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
