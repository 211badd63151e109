"""Microseconds per call of the training transform's launch (csrc/train_transform.hip, ``TrainTransform.detr()``) next to
the same chain written with torch ops on the same device and in the same process: ``flip``, ``F.interpolate(...,
antialias=True)``, the slice, ``round``, the conversion, Normalize, then a ``torch.zeros`` canvas, copies and the mask.

    python benchmarks/train_transform_micro.py [--repeats 7] [--iters 50] [--out FILE.json]

B = 2 uint8 sources of 480 x 640 and 427 x 640, ``TrainTransform.detr()`` forced to each branch (``plain``: one resize;
``crop``: resize -> crop -> resize), the draws fixed by a seed, both images flipped or not as drawn.  Each configuration
runs in a child process of its own under a time limit; the first failure ends the run.  Times are the median over
``--repeats`` windows of ``--iters`` calls, each window timed by device events; the device launches of one call are counted
with the profiler.  The result also holds, per branch, how many two-resize workgroups stage their window of the
intermediate image in LDS and how many recompute it (for the preset: all staged).  If the restatement cannot run on the
device in this torch build, its entries hold the error text and the HIP times stand alone.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SOURCES = ((480, 640), (427, 640))
CONFIGS = {"plain": 0, "crop": 1}


def torch_transform(images, params, canvas_hw):
    """The chain of ``params`` in plain torch ops on the device (uint8 images)."""
    import torch
    import torch.nn.functional as F
    dev = images[0].device
    mean = torch.tensor((0.485, 0.456, 0.406), device=dev).view(3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device=dev).view(3, 1, 1)
    canvas = torch.zeros(len(images), 3, *canvas_hw, device=dev)
    mask = torch.ones(len(images), *canvas_hw, device=dev, dtype=torch.bool)

    def resize(x, size):
        return F.interpolate(x[None], size=size, mode="bilinear", align_corners=False, antialias=True)[0].round()

    for b, (im, p) in enumerate(zip(images, params)):
        x = im.float()
        if p.flip:
            x = x.flip(-1)
        if p.n_stages == 2:
            top, left, ch, cw = p.crop
            x = resize(x, p.size1)[:, top:top + ch, left:left + cw]
        x = resize(x, p.size) / 255
        nh, nw = p.size
        canvas[b, :, :nh, :nw] = (x - mean) / std
        mask[b, :nh, :nw] = False
    return canvas, mask


def worker(name, repeats, iters, seed):
    import torch
    from salience_detr_amd import TrainTransform
    from salience_detr_amd.train_transform import plan_stats
    g = torch.Generator().manual_seed(0)
    images = [(torch.rand(3, h, w, generator=g) * 255).round().to(torch.uint8).cuda() for h, w in SOURCES]
    tf = TrainTransform.detr()
    torch.manual_seed(seed)
    random.seed(seed)
    params = [tf.sample(h, w, branch=CONFIGS[name]) for h, w in SOURCES]
    staged, recomputed = plan_stats(SOURCES, params)

    def hip():
        return tf(images, None, params=params)

    first = hip()
    canvas_hw = tuple(first.canvas.shape[-2:])

    def restated():
        return torch_transform(images, params, canvas_hw)

    def timed(fn):
        for _ in range(5):
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

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

    def attempt(what):
        try:
            return what()
        except Exception as e:      # the restatement's ops may be missing on the device in this build: say so
            return {"error": f"{type(e).__name__}: {e}"[:300]}

    result = {"config": name, "sources": [list(s) for s in SOURCES], "plans": [p.plan() for p in params],
              "canvas": list(canvas_hw), "batch": len(SOURCES), "device": torch.cuda.get_device_name(0), "repeats": repeats,
              "iters": iters, "seed": seed, "two_stage_workgroups": {"staged": staged, "recomputed": recomputed},
              "hip": timed(hip), "hip_launches": attempt(lambda: launches(hip)), "torch": attempt(lambda: timed(restated))}
    if "error" not in result["torch"]:
        result["torch_launches"] = attempt(lambda: launches(restated))
        want = restated()[0]
        std = torch.tensor((0.229, 0.224, 0.225), device=want.device).view(1, 3, 1, 1)
        steps = ((first.canvas - want).abs() * std * 255).round()
        result["pixels_off_torch"] = float((steps != 0).float().mean().item())
        result["largest_step_off_torch"] = float(steps.max().item())
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.repeats, args.iters, args.seed)
        return 0
    results = []
    for name in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", name, "--repeats", str(args.repeats),
               "--iters", str(args.iters), "--seed", str(args.seed)]
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
