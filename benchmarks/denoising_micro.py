"""Microseconds per call of the denoising-query generator (csrc/denoising.hip) next to a plain torch restatement of the
reference formulation (models/bricks/denoising.py:GenerateCDNQueries: ~25 small ops, host-built index tensors, a
``torch.zeros`` pair per call) on the same device and in the same process.

    python benchmarks/denoising_micro.py [--repeats 7] [--iters 200] [--out FILE.json]

B = 2, E = 256, C = 91, 900 matching queries, counts (7, 20) and (1, 100); forward and forward + backward, eager and
replayed from a captured graph (the HIP generator only: the restatement builds index tensors on the host).  Every
configuration runs in a child process of its own under a time limit; the first failure ends the run.  Times are the
median over ``--repeats`` windows of ``--iters`` calls, each window timed by device events.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"7_20": (7, 20), "1_100": (1, 100)}
B, E, C, NQ = 2, 256, 91, 900


def torch_generator(weight, labels_list, boxes_list, groups, max_gt, p_label=0.5, s_box=1.0):
    """The reference formulation in plain torch ops on the device (fresh draws per call)."""
    import torch
    dev = weight.device
    counts = [int(x.numel()) for x in labels_list]
    labels = torch.cat(labels_list).repeat(2 * groups, 1).flatten()
    boxes = torch.cat(boxes_list).repeat(2 * groups, 1)
    flip = torch.rand_like(labels.float()) < p_label * 0.5
    labels = torch.where(flip, torch.randint_like(labels, 0, C), labels)
    n = len(boxes) // groups // 2
    positive = (torch.arange(n, device=dev)[None] + torch.arange(groups, device=dev)[:, None] * 2 * n).flatten()
    half = boxes[:, 2:] / 2
    diff = torch.cat([half, half], -1)
    sign = torch.randint_like(boxes, 0, 2) * 2.0 - 1.0
    part = torch.rand_like(boxes)
    part[positive + n] += 1.0
    part = part * sign
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), -1)
    xyxy = (xyxy + part * diff * s_box).clamp(0.0, 1.0)
    x1, y1, x2, y2 = xyxy.unbind(-1)
    boxes = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), -1)
    boxes = torch.log(boxes.clamp(min=1e-3) / (1 - boxes).clamp(min=1e-3))
    emb = torch.nn.functional.embedding(labels, weight)
    n_dn = 2 * groups * max_gt
    label_q = torch.zeros(len(counts), n_dn, E, device=dev)
    box_q = torch.zeros(len(counts), n_dn, 4, device=dev)
    batch_idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).repeat(2 * groups, 1).flatten()
    valid = torch.cat([torch.arange(c) for c in counts])
    valid = torch.cat([valid + max_gt * i for i in range(2 * groups)]).long()
    label_q[(batch_idx, valid)] = emb
    box_q[(batch_idx, valid)] = boxes
    total = n_dn + NQ
    mask = torch.zeros(total, total, device=dev, dtype=torch.bool)
    mask[n_dn:, :n_dn] = True
    for i in range(groups):
        a, b = 2 * max_gt * i, 2 * max_gt * (i + 1)
        mask[a:b, :a] = True
        mask[a:b, b:n_dn] = True
    return label_q, box_q, mask


def worker(name, repeats, iters):
    import torch
    from salience_detr_amd import denoising as D
    from salience_detr_amd.set_criterion import stage_targets
    counts = CONFIGS[name]
    g = torch.Generator().manual_seed(0)
    targets = [{"boxes": torch.cat([torch.rand(n, 2, generator=g) * 0.6 + 0.2, torch.rand(n, 2, generator=g) * 0.3 + 0.02], -1),
                "labels": torch.randint(0, C, (n,), generator=g)} for n in counts]
    gen = D.GenerateCDNQueries(NQ, C, E).cuda()
    staged = stage_targets(targets, device="cuda")
    max_gt = max(counts)
    groups = D.denoising_groups(100, max_gt)
    labels_dev = [t["labels"].cuda() for t in targets]
    boxes_dev = [t["boxes"].cuda() for t in targets]
    go = torch.randn(B, 2 * groups * max_gt, E, device="cuda")
    weight = gen.label_encoder.weight

    def hip_fwd():
        return gen(None, None, staged=staged)[0]

    def hip_fwd_bwd():
        return torch.autograd.grad(hip_fwd(), weight, go)

    def torch_fwd():
        return torch_generator(weight, labels_dev, boxes_dev, groups, max_gt)[0]

    def torch_fwd_bwd():
        return torch.autograd.grad(torch_fwd(), weight, go)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        windows = []
        for _ in range(repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            end.record()
            torch.cuda.synchronize()
            windows.append(start.elapsed_time(end) * 1000.0 / iters)
        return {"median_us": statistics.median(windows), "min_us": min(windows), "max_us": max(windows)}

    def graphed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay

    result = {"config": name, "counts": counts, "groups": groups, "n_dn": 2 * groups * max_gt,
              "device": torch.cuda.get_device_name(0), "repeats": repeats, "iters": iters,
              "hip_forward": timed(hip_fwd), "hip_forward_backward": timed(hip_fwd_bwd),
              "torch_forward": timed(torch_fwd), "torch_forward_backward": timed(torch_fwd_bwd),
              "hip_forward_graph": timed(graphed(hip_fwd)), "hip_forward_backward_graph": timed(graphed(hip_fwd_bwd))}
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.repeats, args.iters)
        return 0
    results = []
    for name in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, "--repeats", str(args.repeats),
               "--iters", str(args.iters)]
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.step_timeout} s; stopping", flush=True)
            return 1
        if proc.returncode != 0:
            print(f"{name}: exit status {proc.returncode}; stopping\n{proc.stderr[-2000:]}", flush=True)
            return 1
        line = next(l for l in proc.stdout.splitlines() if l.startswith("RESULT "))
        results.append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
