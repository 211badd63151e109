"""Where the detection post-processing launch spends its time, attributed by shape rather than by stamps: each case
changes one thing (row length -> resident vs streamed select, how the logits spread over the first round's histogram
bins, K -> sort / epilogue, filters -> NMS, dtype -> index rounds in tie groups) and the kernel durations come from a
kernel trace of this script.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o pp -- python benchmarks/postprocess_phases.py
    python benchmarks/postprocess_phases.py --summarize OUT/pp_kernel_trace.csv     # one JSON line
"""
import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 20
# (name, Nq, C, dtype, k, spread, conf, nms)
CASES = [
    ("resident_450x91_k300", 450, 91, torch.float32, 300, False, -1, -1),
    ("resident_450x91_k300_spread", 450, 91, torch.float32, 300, True, -1, -1),
    ("streamed_900x91_k300", 900, 91, torch.float32, 300, False, -1, -1),
    ("streamed_900x91_k300_spread", 900, 91, torch.float32, 300, True, -1, -1),
    ("streamed_900x91_k1", 900, 91, torch.float32, 1, False, -1, -1),
    ("streamed_900x91_k1024", 900, 91, torch.float32, 1024, False, -1, -1),
    ("streamed_900x91_k300_conf_nms", 900, 91, torch.float32, 300, False, 0.3, 0.5),
    ("streamed_900x91_k300_bf16", 900, 91, torch.bfloat16, 300, False, -1, -1),
    ("small_100x91_k300", 100, 91, torch.float32, 300, False, -1, -1),
]


def run():
    from salience_detr_amd.post_process import detections_padded
    g = torch.Generator().manual_seed(0)
    B = 2
    for name, nq, c, dtype, k, spread, conf, nms in CASES:
        if spread:   # keys spread over ~400 first-round bins: sign x exponents 2^-100 .. 2^100
            logits = (torch.rand(B, nq, c, generator=g) * 2 - 1) * torch.exp2(torch.randint(-100, 100, (B, nq, c), generator=g).float())
        else:        # the usual detector logits: a few first-round bins hold almost every key
            logits = torch.randn(B, nq, c, generator=g) * 1.2 - 4.5
        logits = logits.to(dtype).cuda()
        boxes = torch.cat([torch.rand(B, nq, 2, generator=g) * 0.8 + 0.1, torch.rand(B, nq, 2, generator=g) * 0.3 + 0.02], -1).cuda()
        sizes = torch.tensor([[800, 1066]] * B).cuda()
        for _ in range(REPS):
            detections_padded(logits, boxes, sizes, k, conf, nms)
        torch.cuda.synchronize()


def summarize(path):
    rows = [r for r in csv.DictReader(open(path)) if "detection_postprocess" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == REPS * len(CASES), len(rows)
    out = {}
    for i, case in enumerate(CASES):
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * REPS:(i + 1) * REPS])
        out[case[0]] = {"median_us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1)}
    print(json.dumps({"bench": "postprocess_phases", "batch": 2, "cases": out}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize")
    a = ap.parse_args()
    summarize(a.summarize) if a.summarize else run()
