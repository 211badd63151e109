"""Training the ChannelMapper (row N7): forward + backward of the HIP training form (``set_train_form("hip")``) against the
torch composite (``"torch"``: ``F.conv2d`` + ``F.group_norm`` and their library backward, bf16 under ``torch.autocast``) on
the same device, in one process.

Shapes: the ``r50`` and ``full`` mapper cases of tests/frontend_cases.py (ResNet50 widths 512 / 1024 / 2048 -> 256, four
levels, B = 2; ``full`` is the 800 x 1344 canvas).  Every input requires grad and every parameter is trainable; the loss is
sum(out * cotangent) with fixed cotangents.  Prints one JSON line per shape:
  <form>_<dt>_us        one forward + backward, HIP events around it and a synchronise after; the median of --iters after
                        --warmup, the two forms timed in turns (torch, hip, torch, ..) so that drift hits both alike
  <form>_<dt>_spread    (p90 - p10) / median of those timings
  grad_distance_<dt>    max over the gradients of max|hip - torch| / max|torch|: the two forms compute the same thing
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frontend_cases as FC  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402
from salience_detr_amd.channel_mapper import ChannelMapper  # noqa: E402


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, (ts[(9 * len(ts)) // 10] - ts[len(ts) // 10]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cases", default="r50,full")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frontend_train_micro: no HIP device (nothing is measured on the CPU)")
    for name in args.cases.split(","):
        cin, cout, num_outs, _, _ = FC.MAPPER_CASES[name]
        feats, _ = FC.mapper_inputs(name)
        xs = [f.cuda().requires_grad_(True) for f in feats]
        m = ChannelMapper(list(cin), cout, num_outs)
        m.load_state_dict(FC.mapper_state(m.state_dict(), name))
        m = m.cuda().train()
        with torch.no_grad():
            cots = [syn.det_rand(f"frontend_train_micro.{name}.{l}", tuple(o.shape)).cuda() - 0.5 for l, o in enumerate(m(xs))]
        res = {"case": name, "batch": xs[0].shape[0], "maps": [list(x.shape[-2:]) for x in xs]}
        for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            m.set_dtype(dt)

            def step(form):
                m.set_train_form(form)
                m.zero_grad(set_to_none=True)
                for x in xs:
                    x.grad = None
                if form == "torch" and dt != torch.float32:
                    with torch.autocast("cuda", dtype=dt):
                        outs = m(xs)
                else:
                    outs = m(xs)
                sum((o.float() * c).sum() for o, c in zip(outs, cots)).backward()

            def grads():
                return [p.grad.clone() for p in m.parameters()] + [x.grad.clone() for x in xs]
            times = {"torch": [], "hip": []}
            for i in range(args.warmup + args.iters):
                for form in ("torch", "hip"):
                    t = one(lambda: step(form))
                    if i >= args.warmup:
                        times[form].append(t)
            for form in ("torch", "hip"):
                res[f"{form}_{tag}_us"], res[f"{form}_{tag}_spread"] = summary(times[form])
            step("torch")
            ref = grads()
            step("hip")
            res[f"grad_distance_{tag}"] = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(grads(), ref))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
