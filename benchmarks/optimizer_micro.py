"""Microseconds per optimizer step: the two-launch HIP step (csrc/optimizer.hip, salience_detr_amd/optimizer.py) next to
``clip_grad_norm_(foreach=True)`` + ``torch.optim.AdamW(fused=True)`` on the same tensors, on the same device, in the same
process.

    python benchmarks/optimizer_micro.py [--repeats 7] [--iters 50] [--lists hot_path,detector] [--out FILE.json]

Parameter lists: ``hot_path`` = the parameters of ``bench.py --mode train`` (``build_hot_path()``); ``detector`` = the whole
``SalienceDETR`` with ResNet-50 at the headline dimensions.  Three timed forms per list: the HIP step eager
(``step()``), the HIP step replayed from a captured graph (``step_captured()`` + ``after_replay()`` between replays is host
work and is timed with it), and the torch form eager.  A window is ``--iters`` steps between two device events; the
figure is the median of ``--repeats`` windows with their min-max.  Bytes: 28 B per element for the update (read g, p, m,
v; write p, m, v) + 4 B for the norm's read of g; the fraction is against 8 TB/s.  Launch counts: the profiler's kernels
per step for the eager forms, the kernel nodes of the captured graph for the replayed one.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12


def parameter_list(name):
    import torch
    if name == "hot_path":
        from salience_detr_amd.hot_path import build_hot_path
        model = build_hot_path()
    else:
        from salience_detr_amd.backbone import ResNetBackbone
        from salience_detr_amd.channel_mapper import ChannelMapper
        from salience_detr_amd.detector import SalienceDETR
        from salience_detr_amd.position_encoding import PositionEmbeddingSine
        from salience_detr_amd.post_process import PostProcess
        from salience_detr_amd.salience_transformer import build_salience_transformer
        backbone = ResNetBackbone("resnet50", return_indices=(1, 2, 3), freeze_indices=())
        model = SalienceDETR(backbone, ChannelMapper([512, 1024, 2048], 256, 4),
                             PositionEmbeddingSine(128, 10000, True, offset=-0.5), build_salience_transformer(with_neck=True),
                             PostProcess(300))
    seen, params = set(), []
    for p in model.parameters():
        if id(p) not in seen and p.dtype == torch.float32:
            seen.add(id(p))
            params.append(torch.nn.Parameter(p.detach().clone().cuda()))
    return params


def windows(fn, iters, repeats):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def kernels_per_step(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def run_list(name, iters, repeats):
    import torch
    from salience_detr_amd import graph_guard
    from salience_detr_amd.optimizer import ClippedAdamW
    params = parameter_list(name)
    elements = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    rec = {"list": name, "tensors": len(params), "elements": elements, "bytes_per_step": 32 * elements}

    hip = ClippedAdamW(params, lr=1e-6, max_norm=0.1)
    rec["hip_eager"] = windows(hip.step, iters, repeats)
    rec["hip_eager"]["kernels_per_step"] = kernels_per_step(hip.step)
    hip.prepare()
    torch.cuda.synchronize()
    graph = graph_guard.new_graph()
    with torch.cuda.graph(graph):
        hip.step_captured()
    rec["graph_nodes"] = graph_guard.assert_replay_safe(graph, "captured optimizer step")
    kernel_nodes = graph_guard.node_types(graph).count(0)          # hipGraphNodeTypeKernel
    if not kernel_nodes:
        raise RuntimeError("optimizer_micro: no graph handle, the captured step's launches could not be counted")

    def replay():
        graph.replay()
        hip.after_replay()
    rec["hip_graph"] = windows(replay, iters, repeats)
    rec["hip_graph"]["kernels_per_step"] = kernel_nodes
    del hip, graph

    ref = torch.optim.AdamW(params, lr=1e-6, weight_decay=1e-4, fused=True)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(params, 0.1, foreach=True)
        ref.step()
    rec["torch_fused"] = windows(torch_step, iters, repeats)
    rec["torch_fused"]["kernels_per_step"] = kernels_per_step(torch_step)
    for form in ("hip_eager", "hip_graph", "torch_fused"):
        rec[form]["fraction_of_8TBps"] = rec["bytes_per_step"] / (rec[form]["median_us"] * 1e-6) / PEAK_BYTES_PER_S
    rec["hip_graph_over_torch"] = rec["hip_graph"]["median_us"] / rec["torch_fused"]["median_us"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lists", default="hot_path,detector")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for name in args.lists.split(","):
        rec = run_list(name, args.iters, args.repeats)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
