"""The RepVGGPluX neck's training-form switch and its fixture, without a GPU: the switch's default and errors, the reason
strings that need no device, the new declarations of the header, and tests/golden/neck_train.npz (the imported reference in
float64) against this project's own ``forward_train`` composite in float64 on the CPU -- which ties the fixture, the
composite and the reference together."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import neck_train_cases as TC  # noqa: E402
from salience_detr_amd import _hip  # noqa: E402
from salience_detr_amd.hip_module import HipModule  # noqa: E402
from salience_detr_amd.salience_neck import RepVGGPluXNetwork, build_neck  # noqa: E402

ROUND_OFF = 1e-11   # float64 round-off of a 60-layer composite on tensors of order 1 .. 100, on the tensor's own scale


def test_switch_default_and_bad_form():
    m = build_neck(32, 3, 4)
    assert isinstance(m, HipModule) and m.train_form == "torch"
    assert m.set_train_form("hip") is m and m.train_form == "hip"
    assert m.set_train_form("torch").train_form == "torch"
    with pytest.raises(ValueError, match="'torch' / 'hip'"):
        m.set_train_form("triton")
    assert not any("train_form" in k for k in m.state_dict())


def test_reasons_that_need_no_device():
    m = build_neck(32, 3, 4).train()
    assert m.hip_train_reason() is None and m.hip_train_form()
    x = [torch.zeros(1, 12, 32)]
    assert "CPU tensor" in m.hip_train_reason(x)
    assert "16-bit rows" in m.hip_train_reason([x[0].bfloat16()])
    assert "not float32" in m.hip_train_reason([x[0].double()])
    assert "eval() mode" in m.eval().hip_train_reason()
    m.train()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert "autocast" in m.hip_train_reason()
    m.pan_blocks[0].conv1[1].momentum = None
    assert "momentum=None" in m.hip_train_reason()
    m.pan_blocks[0].conv1[1].momentum = 0.1
    m.lateral_convs[0][1] = torch.nn.BatchNorm2d(32, affine=False)
    assert "affine BatchNorm" in m.hip_train_reason()
    m = build_neck(32, 2, 4).train()
    m.layer_blocks[0].bottlenecks[0].alpha = torch.nn.Parameter(torch.tensor(1.0))
    assert "alpha" in m.hip_train_reason()
    assert "not float32" in build_neck(32, 2, 4).train().double().hip_train_reason()


def test_hip_form_on_cpu_rows_raises_and_never_falls_back():
    m = build_neck(32, 2, 4).train().set_train_form("hip")
    xs = [torch.zeros(1, 48, 32, requires_grad=True), torch.zeros(1, 12, 32, requires_grad=True)]
    with pytest.raises(RuntimeError, match="'hip' training form cannot run: .*CPU tensor"):
        m.forward_levels(xs, [(6, 8), (3, 4)])


def test_header_declares_the_training_entry_points():
    for name in ("sdetr_neck_bwd_run", "sdetr_neck_bwd_op_run", "sdetr_neck_bn_stats", "sdetr_neck_bn_apply", "sdetr_neck_gate_train"):
        assert name in _hip.SIGNATURES and name in _hip.LAUNCHES
    assert "sdetr_neck_bwd_workspace_bytes" in _hip.SIGNATURES and "sdetr_neck_bwd_workspace_bytes" not in _hip.LAUNCHES
    fields = [f for f, _ in _hip.NeckBwdOpStruct._fields_]
    assert fields[0] == "kind" and {"dz", "x2", "stats2", "dweight2", "ld_dz", "ld_x", "ld_out", "src_height", "alpha"} <= set(fields)


@pytest.mark.parametrize("case", list(TC.CASES))
def test_fixture_equals_the_composite_in_float64(case):
    gold = np.load(TC.GOLDEN)
    m = TC.build(RepVGGPluXNetwork, case).double()
    outs, grads, stats = TC.run(m.forward_train, m, case)
    assert [str(n) for n in gold[f"{case}.names"]] == TC.names(m, case)
    assert [str(n) for n in gold[f"{case}.stats"]] == TC.stat_names(m)

    def same(key, t, scale):
        ref = torch.from_numpy(gold[key])
        err = TC.own_scale(t.reshape(-1)[TC.stored_index(t.numel())], ref, scale)
        assert err <= ROUND_OFF, (key, err)
    for l, o in enumerate(outs):
        same(f"{case}.out:{l}", o, float(gold[f"{case}.outmax:{l}"]))
    for n, t in stats.items():
        same(f"{case}.s:{n}", t, float(gold[f"{case}.smax:{n}"]))
    for n, g in grads.items():
        # (conv_mask.bias: identically zero, round-off in the reference -- on conv_mask.weight's scale, see the GPU test)
        sib = n[:-len("bias")] + "weight" if n.endswith("conv_mask.bias") else n
        same(f"{case}.g:{n}", g, float(gold[f"{case}.max:{sib}"]))
        if sib == n:
            assert abs(g.norm().item() - float(gold[f"{case}.norm:{n}"])) <= ROUND_OFF * float(gold[f"{case}.norm:{n}"])
