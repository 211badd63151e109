"""Microseconds per call of the fused eval preprocessing (csrc/eval_resize.hip: ``batch_images(images, resize=(800, 1333))``,
one launch) next to a plain torch restatement of the reference's eval preprocessing (per image
``F.interpolate(..., mode="bilinear", antialias=True)``, the uint8 round trip, ``/ 255``, Normalize; then a ``torch.zeros``
canvas, copies and the mask) on the same device and in the same process.

    python benchmarks/preprocess_micro.py [--repeats 7] [--iters 50] [--out FILE.json]

B = 2 under (800, 1333): 480 x 640 (stretch, -> 800 x 1066) and 3000 x 4000 (shrink; the reference's float32 size rule
gives 799 x 1066 here), uint8 and float32; eager and replayed from a captured graph.  Every configuration runs in a child
process of its own under a time limit; the first failure ends the run.  Times are the median over ``--repeats`` windows
of ``--iters`` calls, each window timed by device events.  If the restatement cannot run on the device in this torch
build, its entries hold the error text and the HIP times stand alone.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIN_SIZE, MAX_SIZE, B = 800, 1333, 2
CONFIGS = {"stretch_u8": ((480, 640), "u8"), "stretch_f32": ((480, 640), "f32"),
           "shrink_u8": ((3000, 4000), "u8"), "shrink_f32": ((3000, 4000), "f32")}


def torch_preprocess(images, sizes, canvas_hw):
    """The reference's eval preprocessing in plain torch ops on the device."""
    import torch
    import torch.nn.functional as F
    mean = torch.tensor((0.485, 0.456, 0.406), device=images[0].device).view(3, 1, 1)
    std = torch.tensor((0.229, 0.224, 0.225), device=images[0].device).view(3, 1, 1)
    canvas = torch.zeros(len(images), 3, *canvas_hw, device=images[0].device)
    mask = torch.ones(len(images), *canvas_hw, device=images[0].device, dtype=torch.bool)
    for b, (im, (nh, nw)) in enumerate(zip(images, sizes)):
        x = F.interpolate(im.float()[None], size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)[0]
        if im.dtype == torch.uint8:
            x = x.round().to(torch.uint8).float() / 255
        canvas[b, :, :nh, :nw] = (x - mean) / std
        mask[b, :nh, :nw] = False
    return canvas, mask


def worker(name, repeats, iters):
    import torch
    from salience_detr_amd import batch_images, eval_resize_size
    (h, w), dt = CONFIGS[name]
    g = torch.Generator().manual_seed(0)
    images = [torch.rand(3, h, w, generator=g) for _ in range(B)]
    if dt == "u8":
        images = [(i * 255).round().to(torch.uint8) for i in images]
    images = [i.cuda() for i in images]
    sizes = [eval_resize_size(h, w, MIN_SIZE, MAX_SIZE)] * B

    def hip():
        return batch_images(images, resize=(MIN_SIZE, MAX_SIZE))

    canvas_hw = tuple(hip()[0].shape[-2:])

    def restated():
        return torch_preprocess(images, sizes, canvas_hw)

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

    def attempt(make):
        try:
            return timed(make())
        except Exception as e:      # the restatement's ops may be missing on the device in this build: say so
            return {"error": f"{type(e).__name__}: {e}"[:300]}

    result = {"config": name, "image": [h, w], "resized": list(sizes[0]), "canvas": list(canvas_hw), "dtype": dt, "batch": B,
              "device": torch.cuda.get_device_name(0), "repeats": repeats, "iters": iters,
              "hip": timed(hip), "hip_graph": timed(graphed(hip)),
              "torch": attempt(lambda: restated)}
    if "error" not in result["torch"]:
        got, want = hip()[0], restated()[0]
        result["max_abs_difference_from_torch"] = (got - want).abs().max().item()
        result["torch_graph"] = attempt(lambda: graphed(restated))
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--step-timeout", type=int, default=120)
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
