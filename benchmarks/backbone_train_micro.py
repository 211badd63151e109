"""Backbone training step (row N0): ResNet-50, ``freeze_indices=(0,)``, B = 2 on the 800 x 1344 canvas, forward + backward,
the ``"hip"`` training form (csrc/backbone_backward.hip) against the ``"torch"`` composite (F.conv2d autograd; bf16:
under ``torch.autocast``) on the same device, in ONE process, the two forms in turns (A B A B ..: the project's A/B
habit, benchmarks/tree_ab.sh), medians over the rounds.  Prints one JSON line:
  hip_<dt>_us / torch_<dt>_us      eager forward + backward, median over --rounds rounds of --iters steps each
  hip_<dt>_graph_us                the "hip" step captured once and replayed (median of --iters replays)
  hip_<dt>_slowest                 the ten slowest kernel launches of one "hip" step: [kernel, us]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import backbone_cases as BC  # noqa: E402
from salience_detr_amd import graph_guard  # noqa: E402
from salience_detr_amd.backbone import ResNetBackbone  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    canvas, _ = BC.canvas_and_mask([BC.syn.det_rand(f"bench.img{i}", (3, h, w)) for i, (h, w) in enumerate(BC.CASES["full"][2])])
    x = canvas.cuda()
    m = ResNetBackbone("resnet50", return_indices=(1, 2, 3), freeze_indices=(0,))
    m.load_state_dict(BC.state(m.state_dict(), "full"))
    m = m.eval().cuda()
    with torch.no_grad():
        cots = {k: torch.randn_like(v) for k, v in m(x).items()}
    res = {"batch": 2, "canvas": list(x.shape[2:])}

    def step(form, dt):
        m.set_train_form(form)
        if form == "torch" and dt != torch.float32:
            with torch.autocast("cuda", dtype=dt):
                outs = m(x)
        else:
            outs = m(x)
        torch.autograd.backward([outs[k] for k in outs], [cots[k] for k in outs])

    for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        m.set_dtype(dt)
        m.zero_grad(set_to_none=True)
        for form in ("hip", "torch"):
            for _ in range(args.warmup):
                step(form, dt)
        times = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            for form in ("hip", "torch"):
                times[form].append(timed(lambda: step(form, dt), args.iters))
        for form in times:
            res[f"{form}_{tag}_us"] = round(median(times[form]), 1)
            res[f"{form}_{tag}_rounds_us"] = [round(t, 1) for t in times[form]]
        # the "hip" step as one graph
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            step("hip", dt)
            torch.cuda.synchronize()
            graph = graph_guard.new_graph()
            with torch.cuda.graph(graph, stream=stream):
                step("hip", dt)
        torch.cuda.current_stream().wait_stream(stream)
        res[f"hip_{tag}_graph_memset_nodes"] = graph_guard.memset_nodes(graph)
        for _ in range(args.warmup):
            graph.replay()
        res[f"hip_{tag}_graph_us"] = round(median([timed(graph.replay, 1) for _ in range(max(args.iters, 5))]), 1)
        del graph
        if not args.no_profile:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step("hip", dt)
                torch.cuda.synchronize()
            launches = sorted(((e.name, e.device_time_total) for e in prof.events() if e.device_time_total > 0),
                              key=lambda t: -t[1])[:10]
            res[f"hip_{tag}_slowest"] = [[n[:80], round(t, 1)] for n, t in launches]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
