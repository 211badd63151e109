"""The forward and backward plans of the ConvNeXt and Swin training forms as digests, on the CPU: no GPU and no compiled
library.  A refactor of the plan builders leaves every line as it was; point ``--tree`` at a checkout of the commit to
compare with.

The two operand packers of ``HipBackbone`` (the only library calls of plan building) are replaced by stubs that return
small CPU tensors.  One line per plan: the op count, the gradient count (backward plans) and a SHA-256 over the ops in
order: the name, every integer and float field and, of every pointer field, null or (the pointed-into buffer's index in
order of first appearance in the plan, the byte offset into it, the buffer's size in bytes).  Which buffers an op shares
with which other op, and how large they are, is therefore part of the digest; allocation order and addresses are not.  A
backward plan's digest also covers every gradient: its name, the buffer it is a view of, its offset, shape and strides.

    python benchmarks/plan_digest.py [--tree PATH]
"""
import argparse
import bisect
import ctypes
import hashlib
import os
import struct
import sys

import torch

# (label, backbone, case, stochastic_depth_prob, compute dtype, trainable prefixes or None: what freeze_indices leaves)
CASES = [("convnext", c, p, d, None) for c in ("ct1", "ct2") for p, d in ((0.0, torch.float32), (0.3, torch.bfloat16))]
CASES += [("swin", c, 0.2, d, None) for c in ("w7t", "w12t", "lt") for d in (torch.float32, torch.bfloat16)]
CASES += [("convnext", "ct1", 0.0, torch.float32, ("features.5.1.block.5", "features.7.0.layer_scale")),
          ("swin", "w7t", 0.2, torch.float32, ("0.features.5.1.mlp.3", "0.features.6.norm"))]


def stub_packers(base):
    """``HipBackbone._packed`` / ``_packed_rows_dgrad`` without the library: one small buffer per layer and arguments."""
    made = {}

    def packed(self, layer, layout=0, scale=None, scale_bias=True, pad_to=1):
        key = (id(layer), "packed", layout, scale is None, scale_bias, pad_to)
        if key not in made:
            made[key] = (layer, torch.zeros(8, dtype=torch.int16), torch.zeros(-(-layer.weight.shape[0] // pad_to) * pad_to))
        return made[key][1:]

    def packed_rows_dgrad(self, layer, scale=None):
        key = (id(layer), "dgrad", scale is None)
        if key not in made:
            made[key] = (layer, torch.zeros(8, dtype=torch.int16))
        return made[key][1]
    base._packed, base._packed_rows_dgrad = packed, packed_rows_dgrad


def model(backbone, case, sd_prob, dtype, prefixes):
    """The case's module as the tests' ``_model`` helpers build it, in ``train()``."""
    if backbone == "convnext":
        import convnext_train_cases as TC
        from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone
        m = ConvNeXtBackbone(None, return_indices=TC.RETURN, freeze_indices=TC.FREEZE, stochastic_depth_prob=sd_prob,
                             block_setting=[CNBlockConfig(*r) for r in TC.setting(case)])
        shape = (2, 3, 64, 96)
    else:
        import swin_train_cases as TC
        from salience_detr_amd.swin import SwinBackbone
        m = SwinBackbone(None, return_indices=TC.RETURN, freeze_indices=TC.FREEZE, **TC.config(case, sd_prob))
        shape = TC.CASES[case][1]
    m.load_state_dict(TC.state(m.state_dict(), case))
    m.train().set_dtype(dtype)
    if prefixes is not None:
        for n, p in m.named_parameters():
            p.requires_grad = n.startswith(prefixes)
    return m, torch.zeros(shape)


def plans(m, x):
    """``(forward (ops, names, buffers), backward (ops, names, buffers), grads)`` of one training step on ``x``."""
    torch.manual_seed(0)
    train = {"first": m._first_trainable()}
    ops, outputs, keep, names = m.build_plan(x, 0, train)
    cots = {k: torch.zeros_like(v) for k, v in outputs.items()}
    bops, bnames, grads, bkeep = m._backward_ops(train["acts"], train["factors"], tuple(x.shape), cots)
    # (the backward also reads the forward's buffers: the stored activations and the stochastic-depth factors)
    return (ops, names, keep), (bops, bnames, list(bkeep) + list(keep) + list(cots.values())), grads


def digest(ops, names, buffers, grads=None) -> str:
    spans = sorted({(s.data_ptr(), s.data_ptr() + s.nbytes()) for s in (t.untyped_storage() for t in buffers) if s.nbytes()})
    starts = [a for a, _ in spans]
    seen, h = {}, hashlib.sha256()
    for op, name in zip(ops, names):
        h.update(name.encode() + b"\0")
        for field, ctype in op._fields_:
            v = getattr(op, field)
            if ctype is ctypes.c_void_p:
                if v is None:
                    h.update(b"null")
                    continue
                i = bisect.bisect_right(starts, v) - 1
                if i < 0 or v >= spans[i][1]:
                    raise SystemExit(f"{name}: {field} points outside every buffer of the plan")
                start, end = spans[i]
                h.update(struct.pack("<qqq", seen.setdefault(start, len(seen)), v - start, end - start))
            else:
                h.update(struct.pack("<d" if ctype in (ctypes.c_float, ctypes.c_double) else "<q", v))
    for name in sorted(grads or {}):   # which op's output a gradient is, and as which view of it
        g = grads[name]
        shape = struct.pack(f"<{2 * g.dim() + 1}q", g.storage_offset(), *g.shape, *g.stride())
        h.update(name.encode() + b"\0" + struct.pack("<q", seen[g.untyped_storage().data_ptr()]) + shape)
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    from salience_detr_amd import backbone_base   # before the tests' case modules, which put their own tree in front
    if os.path.dirname(os.path.dirname(os.path.abspath(backbone_base.__file__))) != tree:
        raise SystemExit(f"salience_detr_amd came from {backbone_base.__file__}, not from {tree}")
    stub_packers(backbone_base.HipBackbone)
    for backbone, case, sd_prob, dtype, prefixes in CASES:
        m, x = model(backbone, case, sd_prob, dtype, prefixes)
        fwd, bwd, grads = plans(m, x)
        tag = f"{case} sd={sd_prob} {str(dtype)[6:]}" + (" partial" if prefixes else "")
        print(f"{tag:28s} forward  {len(fwd[0]):4d} ops            {digest(*fwd)}")
        print(f"{tag:28s} backward {len(bwd[0]):4d} ops {len(grads):3d} grads  {digest(*bwd, grads)}")


if __name__ == "__main__":
    main()
