"""ConvNeXt backbone: the HIP conv_l against the torch composite (F.conv2d / F.layer_norm / F.linear / F.gelu) on the
same device.

conv_l, return_indices (1, 2, 3), B = 2 on an 800 x 1344 canvas, synthetic weights.  Per mode (bf16: HIP 16-bit mode,
torch under torch.autocast; fp32): the two forms timed in turns in one process (eager, median of --iters after --warmup),
then the HIP form under hipGraph replay.  Then every launch of the HIP plan on its own under replay: the ten slowest,
and the sums per op kind.  Prints one JSON line:
  hip_<dt>_us / torch_<dt>_us / hip_<dt>_graph_us     the whole backbone
  mlp_gflop                                           2 M N K of the two Linears of every block + the down-samplers
  hip_<dt>_mlp_us / hip_<dt>_mlp_busy                 the Linear launches' summed time and their MFMA-busy fraction:
                                                      (flop / peak dense rate of the mode's products) / time; fp32 mode
                                                      issues six bf16 products per flop
  hip_<dt>_dwln_us / hip_<dt>_dwln_gbps               the depthwise + LayerNorm launches: time and (read + write) bytes / time
  hip_<dt>_slowest                                    [name, us] of the ten slowest launches
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import convnext_cases as CC  # noqa: E402
from backbone_micro import eager, replayed  # noqa: E402
from salience_detr_amd import _hip  # noqa: E402
from salience_detr_amd.convnext import ConvNeXtBackbone  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 / fp16 matrix rate


def gemm_flops(op):
    if op.kind not in (0, 1):
        return 0.0
    k = op.kernel_size
    return 2.0 * op.batch * (op.height // k) * (op.width // k) * op.out_channels * op.in_channels * k * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--arch", default="conv_l")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    args = ap.parse_args()
    m = ConvNeXtBackbone(args.arch, return_indices=(1, 2, 3))
    m.load_state_dict(CC.state(m.state_dict(), "cnl"))
    m = m.eval().cuda()
    x = CC.syn.det_randn("bench.convnext.canvas", (2, 3, args.height, args.width)).cuda()
    res = {"arch": args.arch, "batch": 2, "canvas": [args.height, args.width]}
    with torch.no_grad():
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            m.set_dtype(dt)

            def composite():
                if dt == torch.float32:
                    return m.forward_torch(x)
                with torch.autocast("cuda", dtype=dt):
                    return m.forward_torch(x)
            hip_ts, torch_ts = [], []
            for _ in range(2):                                   # in turns
                hip_ts.append(eager(lambda: m(x), args.warmup, args.iters))
                torch_ts.append(eager(composite, args.warmup, args.iters))
            res[f"hip_{tag}_us"] = round(min(hip_ts), 1)
            res[f"torch_{tag}_us"] = round(min(torch_ts), 1)
            res[f"hip_{tag}_graph_us"] = round(replayed(lambda: m(x), args.warmup, args.iters), 1)
            ops, _, keep, names = m.build_plan(x)
            lib, prec = m._lib(), m._precision()
            arr = (_hip.ConvnextOpStruct * len(ops))(*ops)
            nbytes = lib.sdetr_convnext_workspace_bytes(arr, len(ops), prec)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
            # warm the stream once (every op reads what its predecessor wrote), then each launch alone; ops that share
            # a shape share a time: measure one per (kind, shape)
            _hip.launch("sdetr_convnext_run", lib, x.device, arr, len(ops), prec, ws.data_ptr(), nbytes)
            seen, times = {}, []
            for i, op in enumerate(ops):
                key = (op.kind, op.in_channels, op.out_channels, op.height, op.width, op.kernel_size, bool(op.out_nchw))
                if key not in seen:
                    one = (_hip.ConvnextOpStruct * 1)(op)
                    seen[key] = replayed(lambda: _hip.check(lib.sdetr_convnext_op_run(_hip.stream_ptr(), one, prec, ws.data_ptr(),
                                                                                      nbytes), "bench", lib), 2, 5)
                times.append(seen[key])
            mlp = [i for i, n in enumerate(names) if n.endswith((".block.3", ".block.5"))]
            dwln = [i for i, o in enumerate(ops) if o.kind == 2]
            mlp_flop = sum(gemm_flops(ops[i]) for i in mlp)
            mlp_us = sum(times[i] for i in mlp)
            res["mlp_gflop"] = round(mlp_flop / 1e9, 1)
            res["gemm_gflop"] = round(sum(gemm_flops(o) for o in ops) / 1e9, 1)
            res[f"hip_{tag}_launches"] = len(ops)
            res[f"hip_{tag}_sum_of_launches_us"] = round(sum(times), 1)
            res[f"hip_{tag}_mlp_us"] = round(mlp_us, 1)
            products = 6.0 if dt == torch.float32 else 1.0
            res[f"hip_{tag}_mlp_busy"] = round(products * mlp_flop / (PEAK_BF16_TFLOPS * 1e6) / mlp_us, 3)
            dw_us = sum(times[i] for i in dwln)
            dw_bytes = sum(ops[i].batch * ops[i].height * ops[i].width * ops[i].in_channels * (4 + (4 if prec == 0 else 2))
                           for i in dwln)
            res[f"hip_{tag}_dwln_us"] = round(dw_us, 1)
            res[f"hip_{tag}_dwln_gbps"] = round(dw_bytes / dw_us / 1e3, 1)
            order = sorted(set((round(times[i], 1), names[i].split(".")[1] + ":" + names[i].split(".", 3)[-1] if ".block." in names[i]
                                else names[i]) for i in range(len(ops))), reverse=True)[:10]
            res[f"hip_{tag}_slowest"] = [[n, t] for t, n in order]
            del keep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
