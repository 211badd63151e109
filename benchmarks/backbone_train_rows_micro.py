"""Forward + backward of the two training forms of a backbone whose stream is rows (ConvNeXt, Swin), in turns in one
process: ``conv_l`` or ``swin_l`` with ``return_indices=(1, 2, 3)``, ``freeze_indices=(0,)`` at B = 2, 800 x 1344, fp32
and bf16.  Prints the median time of a step of the ``"hip"`` form (``csrc/convnext_backward.hip`` /
``csrc/swin_backward.hip``) and of the ``"torch"`` form (the composite ``forward_torch``), then the per-kind times of
one HIP backward (each op of the plan run alone between two events).

    python benchmarks/backbone_train_rows_micro.py --backbone convnext [--steps 10] [--batch 2] [--height 800] [--width 1344] [--arch conv_l]
    python benchmarks/backbone_train_rows_micro.py --backbone swin [--steps 5] [--batch 2] [--height 800] [--width 1344] [--arch swin_l]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from salience_detr_amd import _hip  # noqa: E402
from salience_detr_amd.convnext import ConvNeXtBackbone  # noqa: E402
from salience_detr_amd.swin import SwinBackbone  # noqa: E402

# backbone -> (class, default arch, default steps)
BACKBONES = {"convnext": (ConvNeXtBackbone, "conv_l", 10), "swin": (SwinBackbone, "swin_l", 5)}


def step(m, x, cots):
    m.zero_grad(set_to_none=True)
    outs = m(x)
    sum((outs[k] * cots[k]).sum() for k in outs).backward()


def timed(fn, n):
    times = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def per_kind(m, x, cots):
    """The backward plan of one forward, every op alone: ``{kind label: summed ms}``."""
    outs = m(x)
    state = m._train_state()
    ops, names, _, keep = m._backward_ops(state["acts"], state["factors"], tuple(x.shape), cots)
    lib, precision = m._lib(), m._precision()
    arr = (m.backward_struct * len(ops))(*ops)
    nbytes = getattr(lib, m.backward_prefix + "_workspace_bytes")(arr, len(ops), precision)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    total = {}
    for op, name in zip(ops, names):
        one = (m.backward_struct * 1)(op)
        run = lambda: _hip.launch(m.backward_prefix + "_op_run", lib, x.device, one, precision, ws.data_ptr(), nbytes)
        run()
        label = name[name.index("("):] if "(" in name else name
        if label in ("(wgrad)", "(dgrad)") and ".block.0 " in name:   # (ConvNeXt's depthwise conv)
            label = "(depthwise " + label[1:]
        total[label] = total.get(label, 0.0) + timed(run, 3)
    del outs, keep
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", choices=sorted(BACKBONES), required=True)
    ap.add_argument("--arch")
    ap.add_argument("--steps", type=int)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    args = ap.parse_args()
    cls, arch, steps = BACKBONES[args.backbone]
    arch, steps = args.arch or arch, args.steps or steps
    torch.manual_seed(0)
    x = torch.randn(args.batch, 3, args.height, args.width, device="cuda")
    m = cls(arch, return_indices=(1, 2, 3), freeze_indices=(0,)).cuda().train()
    with torch.no_grad():
        cots = {k: torch.randn_like(v) for k, v in m(x).items()}
    result = {"arch": arch, "shape": list(x.shape), "device": torch.cuda.get_device_name(0)}
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        m.set_dtype(dtype)

        def torch_step():
            if dtype == torch.float32:
                return step(m.set_train_form("torch"), x, cots)
            with torch.autocast("cuda", dtype=dtype):
                return step(m.set_train_form("torch"), x, cots)
        hip_step = lambda: step(m.set_train_form("hip"), x, cots)
        for fn in (hip_step, torch_step):
            fn()
        hip, ref = [], []
        for _ in range(steps):                      # in turns
            hip.append(timed(hip_step, 1))
            ref.append(timed(torch_step, 1))
        result[tag] = {"hip_ms": sorted(hip)[len(hip) // 2], "torch_ms": sorted(ref)[len(ref) // 2]}
        m.set_train_form("hip")
        result[tag]["backward_kinds_ms"] = {k: round(v, 3) for k, v in per_kind(m, x, cots).items()}
        m.zero_grad(set_to_none=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
