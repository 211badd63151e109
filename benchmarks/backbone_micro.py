"""Backbone (row N0): the HIP ResNet-50 against the F.conv2d + frozen-affine composite (MIOpen) on the same device.

B = 2 at 800x1333 and 800x1066 (canvas 800 x 1344), synthetic weights, every figure under hipGraph replay (median of
--iters replays after --warmup).  Prints one JSON line:
  hip_<dt>_us / torch_<dt>_us      the whole backbone (fp32; bf16: HIP 16-bit mode, torch under torch.autocast)
  hip_<dt>_<stage>_us              each stage on its own (stem = conv1 + max pool), its plan slice captured alone
  hip_<dt>_<stage>_tflops          the stage's convolution flops (2 M N K) over its time
  gflop                            convolution flops of the whole backbone, in GFLOP
  detector_<dt>_images_per_s       SalienceDETR(images) (batching -> backbone -> head), eager (its transformer reads
                                   the proposal count on the host, so the detector does not capture as a whole)
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
from salience_detr_amd import _hip, graph_guard  # noqa: E402
from salience_detr_amd.backbone import Bottleneck, ResNetBackbone  # noqa: E402


def replayed(fn, warmup, iters):
    """Median time of one replay of ``fn`` captured in a graph, in us."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
        torch.cuda.synchronize()
        graph = graph_guard.new_graph()
        with torch.cuda.graph(graph, stream=stream):
            fn()
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts.sort()
    return ts[len(ts) // 2]


def eager(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts.sort()
    return ts[len(ts) // 2]


def stage_slices(m):
    """(name, first op, end op) of the stem and every stage in ``build_plan``'s op order."""
    out, i = [("stem", 0, 2)], 2
    for s, stage in enumerate(m.stages()):
        n = sum((3 if isinstance(b, Bottleneck) else 2) + (b.downsample is not None) for b in stage)
        out.append((f"layer{s + 1}", i, i + n))
        i += n
    return out


def conv_flops(op):
    if op.op != 0:
        return 0
    ho = (op.height + 2 * op.padding - op.kernel_size) // op.stride + 1
    wo = (op.width + 2 * op.padding - op.kernel_size) // op.stride + 1
    return 2.0 * op.batch * ho * wo * op.out_channels * op.in_channels * op.kernel_size ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-detector", action="store_true")
    args = ap.parse_args()
    sizes = BC.CASES["full"][2]
    imgs = [BC.syn.det_rand(f"bench.img{i}", (3, h, w)).cuda() for i, (h, w) in enumerate(sizes)]
    canvas, _ = BC.canvas_and_mask([i.cpu() for i in imgs])
    x = canvas.cuda()
    m = ResNetBackbone("resnet50", return_indices=(1, 2, 3))
    m.load_state_dict(BC.state(m.state_dict(), "full"))
    m = m.eval().cuda()
    res = {"batch": 2, "canvas": list(x.shape[2:])}
    with torch.no_grad():
        for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            m.set_dtype(dt)
            res[f"hip_{tag}_us"] = round(replayed(lambda: m(x), args.warmup, args.iters), 1)
            ops, _, keep, _ = m.build_plan(x)
            lib, prec = m._lib(), m._precision()
            total = 0.0
            for name, a, b in stage_slices(m):
                arr = (_hip.BackboneOpStruct * (b - a))(*ops[a:b])
                nbytes = lib.sdetr_backbone_workspace_bytes(arr, b - a, prec)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
                us = replayed(lambda: _hip.check(lib.sdetr_backbone_run(_hip.stream_ptr(), arr, b - a, prec, ws.data_ptr(),
                                                                        nbytes), "bench", lib), args.warmup, args.iters)
                fl = sum(conv_flops(o) for o in ops[a:b])
                total += fl
                res[f"hip_{tag}_{name}_us"] = round(us, 1)
                res[f"hip_{tag}_{name}_tflops"] = round(fl / us / 1e6, 1)
            res["gflop"] = round(total / 1e9, 1)
            res[f"hip_{tag}_tflops"] = round(total / res[f"hip_{tag}_us"] / 1e6, 1)
            del keep

            def composite():
                if dt == torch.float32:
                    return m.forward_torch(x)
                with torch.autocast("cuda", dtype=dt):
                    return m.forward_torch(x)
            res[f"torch_{tag}_us"] = round(replayed(composite, args.warmup, args.iters), 1)
        if not args.no_detector:
            from salience_detr_amd.channel_mapper import ChannelMapper
            from salience_detr_amd.detector import SalienceDETR
            from salience_detr_amd.position_encoding import PositionEmbeddingSine
            from salience_detr_amd.post_process import PostProcess
            from salience_detr_amd.salience_transformer import build_salience_transformer
            det = SalienceDETR(ResNetBackbone("resnet50", return_indices=(1, 2, 3)),
                               ChannelMapper([512, 1024, 2048], 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                               build_salience_transformer(), PostProcess(100))
            det.load_state_dict(BC.syn.det_state_dict(det.state_dict()))
            det = det.eval().cuda()
            for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                det.set_dtype(dt)
                us = eager(lambda: det(imgs), args.warmup, args.iters)
                res[f"detector_{tag}_us"] = round(us, 1)
                res[f"detector_{tag}_images_per_s"] = round(2e6 / us, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
