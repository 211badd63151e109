"""Input stage (row N7): the HIP ChannelMapper + masks/positions against the torch composite on the same device.

B = 2 at 800x1333 and 800x1066 (canvas 800 x 1344), ResNet50 widths 512 / 1024 / 2048 -> 256, num_outs 4, fp32 and bf16.
Prints one JSON line:
  hip_<dt>_us / torch_<dt>_us   the whole stage, HIP events around it (median of --iters after --warmup).  torch =
                                F.conv2d + F.group_norm per level (bf16: under torch.autocast), synthetic.sine_position_embedding
                                and F.interpolate masks per level
  hip_<dt>_launch_us            each launch of the HIP stage timed on its own with events (conv, groupnorm, positions)
  hip_launches                  kernel nodes of the stage captured in a hipGraph (counted, not assumed)
  traffic_floor_us              fp32 input read once + features and positions written once, at 8 TB/s
  flop_floor_<dt>_us            the conv flops at the bf16 matrix-core peak (2.5 PFLOP/s dense): six products per
                                multiply-add in fp32 mode (exact three-way split), one in bf16
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frontend_cases as FC  # noqa: E402
from salience_detr_amd import _hip, graph_guard  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402
from salience_detr_amd.channel_mapper import ChannelMapper  # noqa: E402
from salience_detr_amd.position_encoding import PositionEmbeddingSine, level_masks_and_positions  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


BF16_PEAK = 2.5e15          # dense bf16 MFMA FLOP/s of an MI355X (spec)
HBM_BYTES_PER_S = 8e12
KERNEL_NODE = 0             # hipGraphNodeTypeKernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    feats, mask = FC.mapper_inputs("full")
    feats = [f.cuda() for f in feats]
    mask = mask.cuda()
    m = ChannelMapper([512, 1024, 2048], 256, 4)
    m.load_state_dict(FC.mapper_state(m.state_dict(), "full"))
    m = m.eval().cuda()
    pe = PositionEmbeddingSine(128, 10000, True, offset=-0.5).cuda()
    shapes = FC.extra_shapes([tuple(f.shape[-2:]) for f in feats], 4)

    def hip_stage():
        outs = m(feats)
        return outs, level_masks_and_positions(mask, shapes, pe)

    def torch_stage():
        outs = m.forward_torch(feats)
        lm = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in shapes]
        return outs, [syn.sine_position_embedding(x, 128) for x in lm]

    def launches_of_stage():
        """(conv, groupnorm, positions) as three separately timed calls of the same entry points the modules make."""
        outs = [torch.empty(2, 256, h, w, device="cuda") for h, w in shapes]
        levels = [m._level(i, f, o) for i, (f, o) in enumerate(zip(feats, outs[:3]))] + [m._level(3, feats[2], outs[3])]
        arr = (_hip.FrontendLevelStruct * 4)(*levels)
        lib = m._lib()
        nbytes = lib.sdetr_frontend_workspace_bytes(arr, 4, 2, 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        gn = m.convs[0][1]

        def conv():
            _hip.check(lib.sdetr_frontend_conv(_hip.stream_ptr(), arr, 4, 2, 256, m._precision(), ws.data_ptr(), nbytes),
                       "conv", lib)

        def norm():
            _hip.check(lib.sdetr_frontend_groupnorm(_hip.stream_ptr(), arr, 4, 2, 256, gn.num_groups, gn.eps, ws.data_ptr(),
                                                    nbytes), "groupnorm", lib)
        conv()
        norm()
        return {"conv": timed(conv, args.warmup, args.iters), "groupnorm": timed(norm, args.warmup, args.iters),
                "positions": timed(lambda: level_masks_and_positions(mask, shapes, pe), args.warmup, args.iters)}

    def count_launches():
        hip_stage()
        torch.cuda.synchronize()
        graph = graph_guard.new_graph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                hip_stage()
        torch.cuda.current_stream().wait_stream(stream)
        types = graph_guard.node_types(graph)
        return sum(1 for t in types if t == KERNEL_NODE) if types else None

    flops = 0
    for (c, (h, w)) in zip((512, 1024, 2048), shapes):
        flops += 2 * 2 * h * w * c * 256
    flops += 2 * 2 * shapes[3][0] * shapes[3][1] * 2048 * 9 * 256
    in_bytes = sum(f.numel() * 4 for f in feats)
    out_bytes = sum(2 * 256 * h * w * 4 * 2 for h, w in shapes)    # features + positions
    floor_us = (in_bytes + out_bytes) / HBM_BYTES_PER_S * 1e6
    res = {"batch": 2, "canvas": list(mask.shape[1:]), "gflop": flops / 1e9, "traffic_mb": (in_bytes + out_bytes) / 1e6,
           "traffic_floor_us": floor_us, "flop_floor_fp32_us": 6 * flops / BF16_PEAK * 1e6,
           "flop_floor_bf16_us": flops / BF16_PEAK * 1e6}
    with torch.no_grad():
        for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            m.set_dtype(dt)
            res[f"hip_{tag}_us"] = timed(hip_stage, args.warmup, args.iters)
            res[f"hip_{tag}_launch_us"] = launches_of_stage()
            if dt == torch.float32:
                res[f"torch_{tag}_us"] = timed(torch_stage, args.warmup, args.iters)
            else:
                def torch_ac():
                    with torch.autocast("cuda", dtype=dt):
                        return torch_stage()
                res[f"torch_{tag}_us"] = timed(torch_ac, args.warmup, args.iters)
            res[f"hip_{tag}_floor_fraction"] = floor_us / res[f"hip_{tag}_us"]
        res["hip_launches"] = count_launches()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
