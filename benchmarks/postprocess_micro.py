"""Detection post-processing: the one-launch HIP form (salience_detr_amd.post_process.detections_padded) against the
torch composite restated from the reference's PostProcess (models/bricks/post_process.py; NMS by the oracle's restated
greedy loop, since torchvision is absent), timed between device events.  Prints one JSON line.

    python benchmarks/postprocess_micro.py [--iters N] [--launch-only]

--launch-only runs just the HIP launches (for `rocprofv3 --kernel-trace --stats -- python ... --launch-only`)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import salience_ref as R  # noqa: E402
from salience_detr_amd.post_process import detections_padded  # noqa: E402

NQ, C = 900, 91


def composite(logits, boxes, sizes, k, conf, nms):
    """The reference's PostProcess.forward in torch ops (torchvision's box conversion inlined, its nms restated)."""
    prob = logits.sigmoid()
    vals, idx = torch.topk(prob.view(logits.shape[0], -1), k, dim=1)
    q = torch.div(idx, logits.shape[2], rounding_mode="trunc")
    labels = idx % logits.shape[2]
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    xyxy = torch.gather(xyxy, 1, q.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    xyxy = xyxy * torch.stack([img_w, img_h, img_w, img_h], 1)[:, None, :]
    if conf > 0 or nms > 0:
        keep = [v > conf for v in vals] if conf > 0 else [torch.ones_like(v, dtype=torch.bool) for v in vals]
        if nms > 0:
            for i in range(len(keep)):
                m = torch.zeros_like(keep[i])
                m[R.nms_greedy(xyxy[i].cpu(), vals[i].float().cpu(), nms).to(m.device)] = True
                keep[i] = keep[i] & m
        return [(v[m], l[m], b[m]) for v, l, b, m in zip(vals, labels, xyxy, keep)]
    return vals, labels, xyxy


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    rows = []
    for B in (1, 2, 16):
        for dtype in (torch.float32, torch.bfloat16):
            logits = (torch.randn(B, NQ, C, generator=g) * 1.2 - 4.5).to(dtype).cuda()
            boxes = torch.cat([torch.rand(B, NQ, 2, generator=g) * 0.8 + 0.1,
                               torch.rand(B, NQ, 2, generator=g) * 0.3 + 0.02], -1).cuda()
            sizes = torch.tensor([[800, 1066]] * B, dtype=torch.int64).cuda()
            for k in (100, 300):
                for conf, nms in ((-1, -1), (0.3, 0.5)):
                    row = {"B": B, "dtype": str(dtype).split(".")[-1], "k": k, "filtered": conf > 0}
                    row["hip_us"] = 1e3 * time_ms(lambda: detections_padded(logits, boxes, sizes, k, conf, nms), args.iters)
                    if not args.launch_only:
                        it = max(3, args.iters // 10) if nms > 0 else args.iters
                        row["composite_us"] = 1e3 * time_ms(lambda: composite(logits, boxes, sizes, k, conf, nms), it)
                    rows.append(row)
    print(json.dumps({"bench": "postprocess_micro", "Nq": NQ, "C": C, "rows": rows}))


if __name__ == "__main__":
    main()
