"""Swin backbone: the HIP swin_l against the torch composite (F.conv2d / F.layer_norm / F.linear / matmul / softmax) on the
same device, in the same process.

swin_l, return_indices (1, 2, 3), B = 2 on an 800 x 1344 canvas, synthetic weights.  Per mode (bf16: HIP 16-bit mode,
torch under torch.autocast; fp32): the composite eager (median of --iters after --warmup) and the HIP form under hipGraph
replay (median of --iters replays after --warmup), in turns.  Then every launch of the HIP plan on its own under replay
(one per distinct op shape), summed per op class.  Prints one JSON line:
  hip_<dt>_graph_us / hip_<dt>_us / torch_<dt>_us     the whole backbone (graph replay; eager; the composite, eager)
  hip_<dt>_launches / hip_<dt>_sum_of_launches_us
  hip_<dt>_split_us                                   {class: summed us}: gemm, attention, layer_norm, merging
  hip_<dt>_attention_tflops / _gbps                   the attention launches' 4 N 32 flops per (window, head, query) / time
                                                      and their (qkv in + rows out + table) bytes / time
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

import swin_cases as SC  # noqa: E402
from backbone_micro import eager, replayed  # noqa: E402
from salience_detr_amd import _hip  # noqa: E402
from salience_detr_amd.swin import SwinBackbone  # noqa: E402

FAMILY = {0: "gemm", 1: "gemm", 2: "gemm", 3: "layer_norm", 4: "attention", 5: "merging"}


def attention_work(op, esz):
    """(flops, bytes) of one attention launch: both products over the padded windows; qkv in, rows out, the table."""
    n = op.window * op.window
    windows = op.batch * -(-op.height // op.window) * -(-op.width // op.window)
    rows = op.batch * op.height * op.width
    return windows * op.heads * 4 * n * n * 32, rows * 4 * op.in_channels * esz + op.heads * n * n * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--arch", default="swin_l")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    args = ap.parse_args()
    m = SwinBackbone(args.arch, return_indices=(1, 2, 3))
    m.load_state_dict(SC.state(m.state_dict(), "l"))
    m = m.eval().cuda()
    x = SC.syn.det_randn("bench.swin.canvas", (2, 3, args.height, args.width)).cuda()
    res = {"arch": args.arch, "batch": 2, "canvas": [args.height, args.width]}
    with torch.no_grad():
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            m.set_dtype(dt)

            def composite():
                if dt == torch.float32:
                    return m.forward_torch(x)
                with torch.autocast("cuda", dtype=dt):
                    return m.forward_torch(x)
            graph_ts, torch_ts = [], []
            for _ in range(2):                                   # in turns
                graph_ts.append(replayed(lambda: m(x), args.warmup, args.iters))
                torch_ts.append(eager(composite, args.warmup, args.iters))
            res[f"hip_{tag}_graph_us"] = round(min(graph_ts), 1)
            res[f"torch_{tag}_us"] = round(min(torch_ts), 1)
            res[f"hip_{tag}_us"] = round(eager(lambda: m(x), args.warmup, args.iters), 1)
            ops, _, keep, names = m.build_plan(x)
            lib, prec = m._lib(), m._precision()
            arr = (_hip.SwinOpStruct * len(ops))(*ops)
            nbytes = lib.sdetr_swin_workspace_bytes(arr, len(ops), prec)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
            # warm the stream once (every op reads what its predecessor wrote), then each launch alone; ops that share
            # a shape share a time: measure one per shape
            _hip.launch("sdetr_swin_run", lib, x.device, arr, len(ops), prec, ws.data_ptr(), nbytes)
            seen, times = {}, []
            for op in ops:
                key = (op.kind, op.in_channels, op.out_channels, op.height, op.width, op.kernel_size, op.out_f32, op.window,
                       op.shift, bool(op.residual), bool(op.out_nchw))
                if key not in seen:
                    one = (_hip.SwinOpStruct * 1)(op)
                    seen[key] = replayed(lambda: _hip.check(lib.sdetr_swin_op_run(_hip.stream_ptr(), one, prec, ws.data_ptr(),
                                                                                  nbytes), "bench", lib), 2, 5)
                times.append(seen[key])
            split = {}
            for op, t in zip(ops, times):
                split[FAMILY[op.kind]] = split.get(FAMILY[op.kind], 0.0) + t
            res[f"hip_{tag}_launches"] = len(ops)
            res[f"hip_{tag}_sum_of_launches_us"] = round(sum(times), 1)
            res[f"hip_{tag}_split_us"] = {k: round(v, 1) for k, v in split.items()}
            at = [i for i, o in enumerate(ops) if o.kind == 4]
            work = [attention_work(ops[i], 2 if prec else 4) for i in at]
            t_at = sum(times[i] for i in at)
            res[f"hip_{tag}_attention_tflops"] = round(sum(w[0] for w in work) / t_at / 1e6, 2)
            res[f"hip_{tag}_attention_gbps"] = round(sum(w[1] for w in work) / t_at / 1e3, 1)
            order = sorted(set((round(times[i], 1), names[i]) for i in range(len(ops))), reverse=True)[:10]
            res[f"hip_{tag}_slowest"] = [[n, t] for t, n in order]
            del keep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
