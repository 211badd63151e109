"""No GPU: the ChannelMapper's HIP training form (``set_train_form("hip")``) as far as it goes without a device -- the ABI
in the parsed header, the switch and every ineligibility reason without the library being asked for, the forward and
backward plans on CPU tensors with the packers stubbed, and the fixture's names."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import frontend_train_cases as TC
from salience_detr_amd import _hip
from salience_detr_amd.channel_mapper import ChannelMapper

FIELDS = ["kind", "dz", "x", "weight", "scale", "add", "z", "stats", "gamma", "out", "dgamma", "dbeta", "batch", "in_channels",
          "height", "width", "out_channels", "kernel_size", "groups", "splits", "eps"]
KINDS = {"dgrad": 0, "wgrad": 1, "rows": 2, "group norm": 3, "egest": 4}


def test_the_backward_op_and_its_entry_points_are_in_the_parsed_header():
    assert [f for f, _ in _hip.FrontendBwdOpStruct._fields_] == FIELDS
    for name in ("sdetr_frontend_bwd_workspace_bytes", "sdetr_frontend_bwd_op_run", "sdetr_frontend_bwd_run",
                 "sdetr_frontend_groupnorm_train"):
        assert name in _hip.SIGNATURES, name
    assert {"sdetr_frontend_bwd_run", "sdetr_frontend_bwd_op_run", "sdetr_frontend_groupnorm_train"} <= _hip.LAUNCHES
    assert "sdetr_frontend_bwd_workspace_bytes" not in _hip.LAUNCHES
    assert _hip.SIGNATURES["sdetr_frontend_bwd_workspace_bytes"][0] is ctypes.c_int64


def _no_library(*a, **k):
    raise AssertionError("the library was asked for")


def test_set_train_form_and_every_ineligibility_reason_without_the_library(monkeypatch):
    monkeypatch.setattr(_hip, "lib", _no_library)
    m = ChannelMapper([64, 128], 64, 3)
    assert m.train_form == "torch" and m.set_train_form("hip") is m and m.train_form == "hip"
    with pytest.raises(ValueError, match="'torch' / 'hip'"):
        m.set_train_form("triton")
    assert m.hip_train_reason() is None and m.hip_train_form()
    xs = [torch.zeros(1, 64, 4, 4), torch.zeros(1, 128, 2, 2)]
    assert "CPU tensor" in m.hip_train_reason(xs) and not m.hip_train_form(xs)
    with pytest.raises(RuntimeError, match="cannot run: an input is a CPU tensor"):
        m(xs)
    assert "float16" in m.set_dtype(torch.float16).hip_train_reason()
    assert m.set_dtype(torch.bfloat16).hip_train_reason() is None
    narrow = ChannelMapper([64], 12, 1, norm_layer=partial(nn.GroupNorm, 4)).set_train_form("hip")
    assert narrow.hip_form() and "multiple of 8" in narrow.hip_train_reason()
    other = ChannelMapper([48], 64, 1).set_train_form("hip")
    assert not other.hip_form() and "not one the HIP kernels serve" in other.hip_train_reason()
    for bad, x in ((narrow, torch.zeros(1, 64, 4, 4)), (other, torch.zeros(1, 48, 4, 4))):
        with pytest.raises(RuntimeError, match="the 'hip' training form cannot run"):
            bad([x])
    with torch.no_grad():   # nothing needs autograd: the switch does not matter, the inference form refuses the CPU tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.set_dtype(torch.float32)(xs)


def test_the_default_form_is_still_the_torch_composite(monkeypatch):
    monkeypatch.setattr(_hip, "lib", _no_library)
    m = TC.build(ChannelMapper, "x2")
    assert m.train_form == "torch" and ChannelMapper.train_form == "torch"
    xs = [x.requires_grad_(True) for x in TC.inputs("x2")]
    outs = m(xs)
    ref = m.forward_torch(xs)
    assert all(torch.equal(a, b) for a, b in zip(outs, ref)) and outs[0].grad_fn is not None
    sum(o.sum() for o in outs).backward()
    assert all(p.grad is not None for p in m.parameters()) and all(x.grad is not None for x in xs)


def _plans(case, monkeypatch, input_grads=None, frozen=()):
    made = {}
    monkeypatch.setattr(ChannelMapper, "_packed_weight", lambda self, i: made.setdefault(("w", i), torch.zeros(8, dtype=torch.int16)))
    monkeypatch.setattr(ChannelMapper, "_packed_dgrad", lambda self, i: made.setdefault(("d", i), torch.zeros(8, dtype=torch.int16)))
    m = TC.build(ChannelMapper, case)
    for n, p in m.named_parameters():
        p.requires_grad = not n.startswith(tuple(frozen))
    xs = TC.inputs(case)
    state = {}
    calls, outs, keep = m.build_plan(xs, state)
    cots = [torch.zeros_like(o) for o in outs]
    wanted = [True] * len(xs) if input_grads is None else input_grads
    bwd = m.build_backward_plan(state["acts"], cots, wanted)
    return m, xs, (calls, outs, keep), bwd, cots


def _pointers(op):
    return [getattr(op, f) for f, t in op._fields_ if t is ctypes.c_void_p and getattr(op, f) is not None]


def _spans(tensors):
    return sorted({(s.data_ptr(), s.data_ptr() + s.nbytes()) for s in (t.untyped_storage() for t in tensors)})


def _level(name):
    return int(name.split(" ")[0].split(".")[1])


@pytest.mark.parametrize("case", ["t4", "x2"])
def test_the_training_plans_build_on_the_cpu_and_point_into_what_they_keep(case, monkeypatch):
    m, xs, (calls, outs, keep), (ops, names, grads, dxs, bkeep), cots = _plans(case, monkeypatch)
    nin, n_levels = len(xs), len(m.convs)
    assert len(calls) == n_levels - nin and sum(len(levels) for levels, _ in calls) == n_levels
    held = _spans(keep)
    for levels, kept in calls:
        assert len(kept) == 2 * len(levels)
        for lv in levels:
            for p in _pointers(lv):
                assert any(a <= p < b for a, b in held)
        for t in kept:
            assert any(a <= t.data_ptr() < b for a, b in held)
    # the backward also reads the forward's buffers (z, the statistics, the inputs, an extra level's input)
    held = _spans(list(bkeep) + list(keep) + cots)
    assert len(names) == len(ops) == len(set(names))
    for op, name in zip(ops, names):
        assert op.kind == KINDS[name[name.index("(") + 1:-1]], name
        for p in _pointers(op):
            assert any(a <= p < b for a, b in held), name
    written = _spans(bkeep)
    trainable = dict(m.named_parameters())
    assert set(grads) == set(trainable)
    for n, g in grads.items():       # a gradient is a view of what the ops write
        assert g.shape == trainable[n].shape and g.dtype == torch.float32, n
        assert any(a <= g.data_ptr() < b for a, b in written), n
    outputs = {op.out for op in ops} | {op.dgamma for op in ops} | {op.dbeta for op in ops}
    assert all(g.data_ptr() in outputs for g in grads.values())
    for x, dx in zip(xs, dxs):
        assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.data_ptr() in outputs
    # levels from the last to the first, then the egests; one group norm per level
    order = [_level(n) for n in names if n.endswith("(group norm)")]
    assert order == list(reversed(range(n_levels)))
    level_ops = [n for n in names if not n.startswith("input.")]
    assert [_level(n) for n in level_ops] == sorted((_level(n) for n in level_ops), reverse=True)
    assert names[-nin:] == [f"input.{j} (egest)" for j in range(nin)]
    # an extra level's backward-data result is the `add` of the level below; the last input sums two results
    by_name = dict(zip(names, ops))
    for i in range(nin + 1, n_levels):
        assert by_name[f"convs.{i - 1} (group norm)"].add == by_name[f"convs.{i} (dgrad)"].out
    assert by_name[f"convs.{nin - 1} (group norm)"].add is None
    last = by_name[f"input.{nin - 1} (egest)"]
    assert {last.dz, last.add} == {by_name[f"convs.{nin} (dgrad)"].out, by_name[f"convs.{nin - 1} (dgrad)"].out}
    # the last backbone map is turned into rows once, for both levels that read it
    assert f"convs.{nin} (rows)" in names and f"convs.{nin - 1} (rows)" not in names
    assert by_name[f"convs.{nin} (wgrad)"].x == by_name[f"convs.{nin - 1} (wgrad)"].x


def test_the_stored_state_holds_aliases_of_the_returned_maps_never_the_maps(monkeypatch):
    """The autograd node owns the state and the returned maps own the node: a map kept in the state would be a reference
    cycle, and the step's graph (with its gradient accumulators) would live on until a garbage collection."""
    m, xs, (_, outs, _), _, _ = _plans("x2", monkeypatch)
    state = {}
    _, outs, _ = m.build_plan(xs, state)
    acts, nin = state["acts"], len(xs)
    assert all(a is not o for a in acts.values() for o in outs)
    assert sorted(k for k in acts if k.endswith(".out")) == [f"convs.{i}.out" for i in range(nin, len(m.convs) - 1)]
    for i in range(nin, len(m.convs) - 1):
        kept = acts[f"convs.{i}.out"]
        assert kept.data_ptr() == outs[i].data_ptr() and kept.shape == outs[i].shape and not kept.requires_grad
    assert all(acts[f"input.{l}"] is x for l, x in enumerate(xs))     # the inputs are not copied


@pytest.mark.parametrize("case", ["t4", "x2"])
def test_no_backward_data_or_egest_for_an_input_without_grad(case, monkeypatch):
    m, xs, _, (ops, names, grads, dxs, _), _ = _plans(case, monkeypatch, input_grads=[False] * len(TC.CASES[case][0]))
    nin, n_levels = len(xs), len(m.convs)
    assert all(dx is None for dx in dxs) and not any("egest" in n for n in names)
    # only an extra level above a trainable extra level still sends its backward-data down
    assert [n for n in names if "dgrad" in n] == [f"convs.{i} (dgrad)" for i in reversed(range(nin + 1, n_levels))]
    assert set(grads) == {n for n, _ in m.named_parameters()}
    m, xs, _, (ops, names, grads, dxs, _), _ = _plans(case, monkeypatch, input_grads=[True] + [False] * (nin - 1),
                                                      frozen=("convs.1.", f"convs.{n_levels - 1}.0"))
    assert [dx is not None for dx in dxs] == [True] + [False] * (nin - 1)
    assert [n for n in names if "egest" in n] == ["input.0 (egest)"]
    assert "convs.1 (group norm)" not in names and "convs.1.0.weight" not in grads and "convs.1.1.bias" not in grads
    assert f"convs.{n_levels - 1} (wgrad)" not in names and f"convs.{n_levels - 1} (group norm)" in names
    assert set(grads) == {n for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("case", list(TC.CASES))
def test_the_fixture_names_are_the_module_s_trainable_parameters_and_inputs(case):
    gold = np.load(TC.GOLDEN)
    m = TC.build(ChannelMapper, case)
    names = [str(n) for n in gold[f"{case}.names"]]
    params = [n for n, p in m.named_parameters() if p.requires_grad]
    assert names == params + [f"input.{l}" for l in range(len(TC.CASES[case][0]))]
    for n in names:
        numel = dict(m.named_parameters())[n].numel() if n in params else TC.inputs(case)[int(n[-1])].numel()
        assert gold[f"{case}.g:{n}"].shape == (min(numel, TC.STORE),) and gold[f"{case}.g:{n}"].dtype == np.float64
        for key in ("norm", "max", "d32", "dbf16"):
            assert np.isfinite(gold[f"{case}.{key}:{n}"]), (key, n)
    for k, v in m.state_dict().items():
        if k.endswith(".1.weight"):
            assert (v[list(TC.ZERO_GAMMA)] == 0).all() and (v != 0).sum() == v.numel() - len(TC.ZERO_GAMMA)
