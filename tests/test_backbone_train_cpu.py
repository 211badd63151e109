"""CPU: the backbone's "hip" training form, host side.  G1 ties the float64 masked restatement (this project's modules,
every ReLU replaced by ``x * mask``, tests/backbone_train_cases.walk), which is the GPU tests' oracle, to the imported
reference's gradients in tests/golden/backbone_train.npz; the rest checks the switch, the eligibility predicate and the
backward plan, none of which needs the library."""
from collections import Counter

import numpy as np
import pytest
import torch

import backbone_cases as BC
import backbone_train_cases as TC
from salience_detr_amd.backbone import ResNetBackbone


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


def _model(case):
    arch, ret, _ = BC.CASES[case]
    m = ResNetBackbone(arch, return_indices=ret, freeze_indices=TC.FREEZE)
    m.load_state_dict(BC.state(m.state_dict(), case))
    return m.eval()


@pytest.mark.parametrize("case", TC.CASES)
def test_g1_masked_restatement_reproduces_the_reference_gradients(gold, case):
    m = _model(case).double()
    names = [str(n) for n in gold[f"{case}.names"]]
    assert names == TC.trainable_names(m, m.num_stages) == [n + ".weight" for n, _ in m._trainable_convs()]
    masks = TC.unpack_masks(gold[f"{case}.masks"], gold[f"{case}.mask_shapes"])
    canvas, _ = BC.canvas_and_mask(BC.images(case))
    got = TC.masked_grads(m, canvas, m.num_stages, m.return_indices, names, case, masks=masks)
    for n in names:
        ref = torch.from_numpy(gold[f"{case}.g:{n}"])
        g = got[n].reshape(-1)[TC.stored_index(got[n].numel())]
        assert TC.own_scale(g, ref, float(gold[f"{case}.max:{n}"])) <= 1e-10, n
        assert abs(got[n].norm().item() - float(gold[f"{case}.norm:{n}"])) <= 1e-10 * float(gold[f"{case}.norm:{n}"]), n


def test_train_form_switch_and_default():
    m = ResNetBackbone("resnet18", freeze_indices=(0,))
    assert m.train_form == "torch"
    assert m.set_train_form("hip") is m and m.train_form == "hip"
    assert m.set_train_form("torch").train_form == "torch"
    with pytest.raises(ValueError):
        m.set_train_form("triton")


def test_eligibility_and_reasons():
    for arch in ("resnet18", "resnet50"):
        assert ResNetBackbone(arch, return_indices=(1, 2, 3), freeze_indices=(0,)).hip_train_form()
    m = ResNetBackbone("resnet18")
    assert not m.hip_train_form() and "stem" in m.hip_train_reason()
    m = ResNetBackbone("resnext50_32x4d", freeze_indices=(0,))
    assert not m.hip_train_form() and "architecture" in m.hip_train_reason()
    m = ResNetBackbone("resnet18", freeze_indices=(0,)).set_dtype(torch.float16)
    assert not m.hip_train_form() and "float16" in m.hip_train_reason()
    m = ResNetBackbone("resnet18", freeze_indices=(0,))
    x = torch.zeros(1, 3, 32, 32, requires_grad=True)
    assert m.hip_train_form() and not m.hip_train_form(x) and "input" in m.hip_train_reason(x)
    # a "hip" request that is not eligible raises at forward, naming the reason: never a silent fallback
    with pytest.raises(RuntimeError, match="input requires a gradient"):
        m.set_train_form("hip")(x)
    with pytest.raises(RuntimeError, match="stem"):
        ResNetBackbone("resnet18").set_train_form("hip")(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("arch,wgrad,dgrad", [("resnet50", 42, 40), ("resnet18", 15, 13)])
def test_backward_plan(arch, wgrad, dgrad):
    m = ResNetBackbone(arch, return_indices=(1, 2, 3), freeze_indices=(0,))
    plan = m.build_backward_plan(2, 64, 96)
    kinds = Counter(d["kind"] for d in plan)
    assert kinds == {"wgrad": wgrad, "dgrad": dgrad, "ingest": 3}
    trainable = [n for n, _ in m._trainable_convs()]
    assert sorted(d["conv"] for d in plan if d["kind"] == "wgrad") == sorted(trainable)   # each exactly once
    assert all(not n.startswith("layer1.") and n != "conv1" for n in trainable)
    # nothing reads or writes a gradient of the frozen prefix: its first consumers get no dgrad
    first = [n for n in trainable if n.startswith("layer2.0.") and (n.endswith("conv1") or "downsample" in n)]
    assert len(first) == 2 and not any(d["kind"] == "dgrad" and d["conv"] in first for d in plan)
    # every gradient buffer is written exactly once, before it is read
    written = set()
    for d in plan:
        for operand in ("dz", "add"):
            if d[operand] is not None and not d[operand].startswith("cot:"):
                assert d[operand] in written, (d["conv"], operand)
        assert d["out"] not in written
        written.add(d["out"])
    # a tensor with two consumers (a block's input: first conv + identity / downsample) gets exactly one `add`
    blocks = [b for b in m._blocks(64, 96) if b["input_needs"]]
    for b in blocks:
        target = ("raw:" if b["input_returned"] else "dz:") + b["input"]
        producers = [d for d in plan if d["out"] == target]
        assert len(producers) == 1 and producers[0]["add"] is not None and producers[0]["kind"] == "dgrad"
    assert sum(d["add"] is not None for d in plan if d["kind"] == "dgrad") == len(blocks)
    # a returned stage that feeds the next one: its ingest adds the raw gradient the next stage produced
    ingests = {d["conv"]: d for d in plan if d["kind"] == "ingest"}
    assert ingests["layer4"]["add"] is None and ingests["layer3"]["add"] is not None and ingests["layer2"]["add"] is not None
    assert all(d["mask"] is not None for d in ingests.values())


def test_frozen_convs_inside_a_trainable_stage_get_no_wgrad_but_pass_gradients():
    m = ResNetBackbone("resnet18", return_indices=(1, 2, 3), freeze_indices=(0,))
    m.layer3[0].conv2.weight.requires_grad = False
    plan = m.build_backward_plan(1, 64, 64)
    assert not any(d["kind"] == "wgrad" and d["conv"] == "layer3.0.conv2" for d in plan)
    assert any(d["kind"] == "dgrad" and d["conv"] == "layer3.0.conv2" for d in plan)
    assert Counter(d["kind"] for d in plan) == {"wgrad": 14, "dgrad": 13, "ingest": 3}
