"""COCO box evaluation (salience_detr_amd.coco_eval): the update launch per batch, and accumulate + summarize over a
synthetic val-sized record set, HIP against the torch composite on the CPU for scale.  Prints one JSON line.

    python benchmarks/coco_eval_micro.py [--iters N] [--images 5000] [--skip-cpu]

update: 2 images x 300 detections over 80 categories, 8 ground truths per image, timed between device events (inputs
already padded on the device).  accumulate + summarize: 5000 images x 100 detections, 80 categories, synthetic matched /
ignored bits, wall clock around both calls with a device sync (the two sorts and the copy of the arrays to the host are
inside)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from salience_detr_amd import coco_eval as E  # noqa: E402

K = 80


def update_inputs(g, B=2, k=300, G=8):
    xy = torch.rand(B, k, 2, generator=g) * 500
    boxes = torch.cat([xy, xy + torch.rand(B, k, 2, generator=g) * 200 + 4], -1)
    gt_boxes = boxes[:, :G] + torch.rand(B, G, 4, generator=g) * 6
    gt_labels = torch.randint(0, K, (B, G), generator=g)
    labels = torch.randint(0, K, (B, k), generator=g)
    labels[:, :G * 4] = gt_labels.repeat(1, 4)                      # several detections around every ground truth
    boxes[:, :G * 4] = gt_boxes.repeat(1, 4, 1) + torch.rand(B, G * 4, 4, generator=g) * 20
    area = ((gt_boxes[..., 2] - gt_boxes[..., 0]) * (gt_boxes[..., 3] - gt_boxes[..., 1])).double()
    return (torch.rand(B, k, generator=g), labels, boxes, torch.full((B,), k, dtype=torch.int32), gt_boxes, gt_labels, area,
            torch.zeros(B, G, dtype=torch.uint8), torch.full((B,), G, dtype=torch.int32), torch.arange(B))


def synthetic_records(g, images, per_image=100):
    n = images * per_image
    image = torch.arange(images).repeat_interleave(per_image)
    cat = torch.randint(0, K, (n,), generator=g)
    order = torch.sort(image * K + cat, stable=True).indices
    image, cat = image[order], cat[order]
    rank = torch.arange(n) - torch.searchsorted(image * K + cat, image * K + cat)
    score = torch.rand(n, generator=g).double().view(torch.int64)
    matched = torch.randint(0, 1 << 40, (n,), generator=g) & torch.randint(0, 1 << 40, (n,), generator=g)
    ignored = matched & torch.randint(0, 1 << 40, (n,), generator=g) & torch.randint(0, 1 << 40, (n,), generator=g)
    det = torch.stack([image, cat | (rank << 32), score, matched, ignored], 1)
    pairs = torch.unique(image * K + cat)
    counts = torch.randint(1, 4, (pairs.numel(), 1), generator=g)
    gt = torch.cat([(pairs // K)[:, None], (pairs % K)[:, None], counts.expand(-1, 4), counts], 1)
    return det, gt


def timed_summary(det, gt, device, iters):
    best = None
    for _ in range(iters):
        ev = E.CocoBoxEvaluator(range(K), device=device)
        ev._batches = [(det, gt, None)]
        if device == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.accumulate()
        stats = ev.summarize(verbose=False)
        if device == "cuda":
            torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        best = dt if best is None else min(best, dt)
    return best, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    out = {"bench": "coco_eval_micro", "categories": K}

    ev = E.CocoBoxEvaluator(range(K), device="cuda")
    lut, thr, _ = ev._constants()
    inputs = tuple(t.cuda().contiguous() for t in update_inputs(g))
    for _ in range(3):
        E.hip_update(*inputs, lut, K, thr)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        E.hip_update(*inputs, lut, K, thr)
    b.record()
    torch.cuda.synchronize()
    out["update_us_per_batch_2x300"] = 1e3 * a.elapsed_time(b) / args.iters

    det, gt = synthetic_records(g, args.images)
    out["records"] = det.shape[0]
    timed_summary(det.cuda(), gt.cuda(), "cuda", 1)                  # warm-up
    out["accumulate_summarize_ms_hip"], stats = timed_summary(det.cuda(), gt.cuda(), "cuda", 3)
    if not args.skip_cpu:
        out["accumulate_summarize_ms_cpu_composite"], cpu_stats = timed_summary(det, gt, "cpu", 1)
        out["max_abs_stat_difference"] = float((stats - cpu_stats).abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
