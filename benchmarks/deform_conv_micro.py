"""The two ops of a DCN conv2 (the exact offset / mask conv, op 3, and the deformable product, op 2) against the plain
3x3 conv (op 0) on the same shapes: ResNet-50 layer2 .. layer4 conv2 at B = 2, canvas 800 x 1344, first (stride 2) and
later (stride 1) blocks.  Every figure is the median over --iters hipGraph replays (after --warmup) of a plan of --repeat
copies of the op, divided by --repeat.  Offsets are N(0, 1 px), mask logits N(0, 1).  Prints one JSON line:
  <shape>_<dt>_plain_us / _offset_us / _deform_us     one launch each
  <shape>_<dt>_ratio                                  (offset + deform) / plain: what a DCN conv2 costs over a plain one
  <shape>_<dt>_deform_ratio                           deform / plain: the gather against the contiguous loader
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from salience_detr_amd import _hip  # noqa: E402
from benchmarks.backbone_micro import replayed  # noqa: E402

SHAPES = [  # (name, channels, input H, input W, stride)
    ("layer2.0", 128, 200, 336, 2), ("layer2.1", 128, 100, 168, 1),
    ("layer3.0", 256, 100, 168, 2), ("layer3.1", 256, 50, 84, 1),
    ("layer4.0", 512, 50, 84, 2), ("layer4.1", 512, 25, 42, 1),
]


def pack(lib, w, beta, precision):
    co, ci = w.shape[:2]
    packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, 3, precision) // 2, dtype=torch.int16, device="cuda")
    bias = torch.empty(co, device="cuda")
    one, zero = torch.ones(co, device="cuda"), torch.zeros(co, device="cuda")
    _hip.check(lib.sdetr_backbone_pack(_hip.stream_ptr(), w.data_ptr(), one.data_ptr(), beta.data_ptr(), zero.data_ptr(),
                                       one.data_ptr(), 0.0, co, ci, 3, 0, precision, packed.data_ptr(), bias.data_ptr()),
               "pack", lib)
    return packed, bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    lib, res, B = _hip.lib(), {"batch": 2, "repeat": args.repeat}, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, c, h, w, s in SHAPES:
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        for precision, tag in ((0, "fp32"), (1, "bf16")):
            act = torch.float32 if precision == 0 else torch.bfloat16
            x = torch.randn(B, h, w, c, generator=g, device="cuda").to(act)
            wt = torch.randn(c, c, 3, 3, generator=g, device="cuda") / (c * 9) ** 0.5
            w_om = torch.zeros(32, c, 3, 3, device="cuda")
            w_om[:27] = torch.randn(27, c, 3, 3, generator=g, device="cuda") / (c * 9) ** 0.5
            om = torch.randn(B, ho, wo, 32, generator=g, device="cuda")
            packed, bias = pack(lib, wt, torch.zeros(c, device="cuda"), precision)
            om_packed, om_bias = pack(lib, w_om, torch.zeros(32, device="cuda"), 0)
            out = torch.empty(B, ho, wo, c, dtype=act, device="cuda")
            om_out = torch.empty(B, ho, wo, 32, device="cuda")
            shape = dict(x=x.data_ptr(), batch=B, in_channels=c, height=h, width=w, kernel_size=3, stride=s, padding=1)
            ops = {
                "plain": dict(op=0, weight=packed.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(), out_channels=c, relu=1),
                "offset": dict(op=3, weight=om_packed.data_ptr(), bias=om_bias.data_ptr(), out=om_out.data_ptr(), out_channels=32),
                "deform": dict(op=2, weight=packed.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(), out_channels=c, relu=1,
                               offset_mask=om.data_ptr()),
            }
            us = {}
            for kind, fields in ops.items():
                arr = (_hip.BackboneOpStruct * args.repeat)(*[_hip.BackboneOpStruct(**shape, **fields)] * args.repeat)
                nbytes = lib.sdetr_backbone_workspace_bytes(arr, args.repeat, precision)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
                total = replayed(lambda: _hip.check(lib.sdetr_backbone_run(_hip.stream_ptr(), arr, args.repeat, precision,
                                                                           ws.data_ptr(), nbytes), "bench", lib),
                                 args.warmup, args.iters)
                us[kind] = total / args.repeat
                res[f"{name}_{tag}_{kind}_us"] = round(us[kind], 1)
            res[f"{name}_{tag}_ratio"] = round((us["offset"] + us["deform"]) / us["plain"], 2)
            res[f"{name}_{tag}_deform_ratio"] = round(us["deform"] / us["plain"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
