"""The forward and backward plans of the ConvNeXt, Swin, ChannelMapper and ResNet training forms as digests, on the CPU: no
GPU and no compiled library.  A refactor of the plan builders leaves every line as it was; point ``--tree`` at a checkout
of the commit to compare with.

ConvNeXt and Swin: the two operand packers of ``HipBackbone`` (the only library calls of their plan building) are replaced
by stubs that return small CPU tensors.  ChannelMapper and ResNet, whose packers and runners differ between trees, are
stubbed at the library boundary instead (``_hip.launch`` does nothing, ``_hip.lib()`` answers every ``*_bytes`` query with
a small constant) and their backward ops are taken where they are handed over for launching: at ``_run_plan``, or at the
``sdetr_frontend_bwd_run`` launch of a mapper that runs its plan itself.  One line per plan: the op count, the gradient count (backward plans) and a SHA-256 over the ops in
order: the name, every integer and float field and, of every pointer field, null or (the pointed-into buffer's index in
order of first appearance in the plan, the byte offset into it, the buffer's size in bytes).  Which buffers an op shares
with which other op, and how large they are, is therefore part of the digest; allocation order and addresses are not.  A
backward plan's digest also covers every gradient (the mapper's input gradients too): its name, the buffer it is a view
of, its offset, shape and strides.

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
# ChannelMapper: (case of frontend_train_cases, setting); "all": everything trainable, every input requires grad;
# "frozen convs": only the GroupNorms trainable, only the last input requires grad
MAPPER_CASES = [(c, s) for c in ("t4", "x2", "g16", "r50") for s in ("all", "frozen convs")]
# ResNet: (case of backbone_train_cases, setting); "all": nothing frozen above the stem; "freeze 0": freeze_indices=(0,);
# "one conv": only layer3.0.conv2 trainable
RESNET_CASES = [(c, s) for c in ("r18", "r50") for s in ("all", "freeze 0", "one conv")]
DTYPES = (torch.float32, torch.bfloat16)
TORCH = {name: getattr(torch, name) for name in ("empty", "zeros", "ones", "empty_like", "zeros_like")}


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


class Boundary:
    """The library boundary without a library, and a record of what crosses it: ``handed`` receives every op list that
    reaches ``_run_plan`` or the ``sdetr_frontend_bwd_run`` launch, ``made`` every tensor allocated meanwhile (a runner's
    buffers are its locals: they have to outlive it for the digest to know their sizes)."""

    def __init__(self, _hip):
        self.handed, self.made = [], []
        _hip.lib = lambda act=None: self
        _hip.launch = self.launch
        for name in TORCH:
            setattr(torch, name, self.recording(TORCH[name]))

    def __getattr__(self, name):
        if name.endswith("_bytes"):
            return lambda *a: 64
        raise AttributeError(name)

    def launch(self, name, act, device, *args, what=None):
        if name == "sdetr_frontend_bwd_run":
            self.made.append(args[0])
            self.handed.append(list(args[0]))

    def run_plan(self, struct_type, c_prefix, ops, device):
        self.handed.append(list(ops))

    def recording(self, fn):
        def allocate(*a, **k):
            t = fn(*a, **k)
            self.made.append(t)
            return t
        return allocate

    def tensors(self):
        return [t for t in self.made if isinstance(t, torch.Tensor)]


def mapper_plans(boundary, case, setting, dtype):
    """``(forward (ops, names, buffers, pointers), backward (ops, names, buffers), grads)`` of one ChannelMapper step."""
    import frontend_train_cases as TC
    from salience_detr_amd.channel_mapper import ChannelMapper
    m = TC.build(ChannelMapper, case).set_dtype(dtype)
    xs = TC.inputs(case)
    wanted = [True] * len(xs)
    if setting == "frozen convs":
        for n, p in m.named_parameters():
            p.requires_grad = not n.endswith(".0.weight")
        wanted = [False] * (len(xs) - 1) + [True]
    m._run_plan = boundary.run_plan
    names = []
    build = m.build_backward_plan
    m.build_backward_plan = lambda *a, **k: names.append(build(*a, **k)) or names[-1]
    state = {}
    calls, outs, keep = m.build_plan(xs, state)
    levels = [lv for lvs, _ in calls for lv in lvs]
    kept = [(f"call{c}.kept{j}", t.data_ptr()) for c, (_, ts) in enumerate(calls) for j, t in enumerate(ts)]
    cots = [torch.zeros_like(o) for o in outs]
    grads, dxs = m._run_backward(state, cots, wanted, 0)
    grads = dict(grads, **{f"input.{j}": dx for j, dx in enumerate(dxs) if dx is not None})
    buffers = boundary.tensors() + list(keep) + cots
    return (levels, [f"convs.{i}" for i in range(len(levels))], keep, kept), (boundary.handed[-1], names[-1][1], buffers), grads


def resnet_plans(boundary, case, setting, dtype):
    """``(forward (ops, names, buffers), backward (ops, names, buffers), grads)`` of one ResNet training step."""
    import backbone_cases as BC
    import backbone_train_cases as TC
    from salience_detr_amd.backbone import ResNetBackbone
    arch, ret, _ = BC.CASES[case]
    m = ResNetBackbone(arch, return_indices=ret, freeze_indices=TC.FREEZE)
    m.load_state_dict(BC.state(m.state_dict(), case))
    m.eval().set_dtype(dtype)
    if setting != "freeze 0":
        for n, p in m.named_parameters():
            p.requires_grad = not n.startswith("conv1.") if setting == "all" else n == "layer3.0.conv2.weight"
    x = torch.zeros(2, 3, 64, 96)
    m._run_plan = boundary.run_plan
    records = []
    build = m.build_backward_plan
    m.build_backward_plan = lambda *a, **k: records.append(build(*a, **k)) or records[-1]
    state = {"acts": {}}
    ops, outputs, keep, names = m.build_plan(x, 0, state["acts"])
    cots = {k: torch.zeros_like(v) for k, v in outputs.items()}
    grads = m._run_backward(state, tuple(x.shape), cots, 0)
    bnames = [f"{d['conv']} ({d['kind']})" for d in records[-1]]
    return (ops, names, keep), (boundary.handed[-1], bnames, boundary.tensors() + list(keep) + list(cots.values())), grads


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


def digest(ops, names, buffers, grads=None, pointers=()) -> str:
    """``pointers``: ``(name, address)`` of what a plan hands over beside its ops; digested as a pointer field is."""
    spans = sorted({(s.data_ptr(), s.data_ptr() + s.nbytes()) for s in (t.untyped_storage() for t in buffers) if s.nbytes()})
    starts = [a for a, _ in spans]
    seen, h = {}, hashlib.sha256()

    def pointer(name, field, v):
        i = bisect.bisect_right(starts, v) - 1
        if i < 0 or v >= spans[i][1]:
            raise SystemExit(f"{name}: {field} points outside every buffer of the plan")
        start, end = spans[i]
        h.update(struct.pack("<qqq", seen.setdefault(start, len(seen)), v - start, end - start))
    for op, name in zip(ops, names):
        h.update(name.encode() + b"\0")
        for field, ctype in op._fields_:
            v = getattr(op, field)
            if ctype is ctypes.c_void_p:
                if v is None:
                    h.update(b"null")
                else:
                    pointer(name, field, v)
            else:
                h.update(struct.pack("<d" if ctype in (ctypes.c_float, ctypes.c_double) else "<q", v))
    for name, v in pointers:
        h.update(name.encode() + b"\0")
        pointer(name, "address", v)
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
    from salience_detr_amd import _hip, backbone_base   # before the tests' case modules, which put their own tree in front
    if os.path.dirname(os.path.dirname(os.path.abspath(backbone_base.__file__))) != tree:
        raise SystemExit(f"salience_detr_amd came from {backbone_base.__file__}, not from {tree}")
    stub_packers(backbone_base.HipBackbone)
    for backbone, case, sd_prob, dtype, prefixes in CASES:
        m, x = model(backbone, case, sd_prob, dtype, prefixes)
        fwd, bwd, grads = plans(m, x)
        tag = f"{case} sd={sd_prob} {str(dtype)[6:]}" + (" partial" if prefixes else "")
        print(f"{tag:28s} forward  {len(fwd[0]):4d} ops            {digest(*fwd)}")
        print(f"{tag:28s} backward {len(bwd[0]):4d} ops {len(grads):3d} grads  {digest(*bwd, grads)}")
    for label, cases, plans_of in (("mapper", MAPPER_CASES, mapper_plans), ("resnet", RESNET_CASES, resnet_plans)):
        for case, setting in cases:
            for dtype in DTYPES:
                fwd, bwd, grads = plans_of(Boundary(_hip), case, setting, dtype)
                tag = f"{label} {case} {setting} {str(dtype)[6:]}"
                print(f"{tag:36s} forward  {len(fwd[0]):4d} ops            {digest(*fwd[:3], None, *fwd[3:])}")
                print(f"{tag:36s} backward {len(bwd[0]):4d} ops {len(grads):3d} grads  {digest(*bwd, grads)}")


if __name__ == "__main__":
    main()
