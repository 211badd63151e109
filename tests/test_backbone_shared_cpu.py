"""CPU: what the four backbones take from ``HipBackbone`` and, with the ChannelMapper, from ``HipModule`` below it, since
the training interface moved there: the interface is the base's own, one autograd node serves every module, a backbone that cannot serve the ``"hip"`` form refuses it with a reason instead of running something
else, the ResNet loads checkpoints through the base's ``load_weights``, and the ConvNeXt and Swin backward plans come
from the base's ``BackwardPlanBuilder``."""
import ast
import ctypes
import os

import pytest
import torch

import convnext_train_cases as CT
import swin_train_cases as ST
from salience_detr_amd import _hip, hip_module
from salience_detr_amd.backbone import ResNetBackbone
from salience_detr_amd.backbone_base import HipBackbone
from salience_detr_amd.channel_mapper import ChannelMapper
from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone
from salience_detr_amd.focalnet import FocalNetBackbone
from salience_detr_amd.hip_module import HipModule
from salience_detr_amd.swin import SwinBackbone

SHARED = ("set_train_form", "hip_train_reason", "hip_train_form", "forward", "forward_hip_train", "_train_state",
          "load_weights", "_check_image")


@pytest.mark.parametrize("cls", [ResNetBackbone, ConvNeXtBackbone, FocalNetBackbone, SwinBackbone])
def test_the_training_interface_is_the_base_class_s(cls):
    for name in SHARED:
        assert getattr(cls, name) is getattr(HipBackbone, name), name
    assert "train_form" not in cls.__dict__ and HipBackbone.train_form == "torch"


MODULE_SHARED = ("set_dtype", "set_train_form", "hip_train_form", "_train_state", "_run_plan", "_precision", "_lib")


def test_the_channel_mapper_takes_the_interface_from_hip_module_as_the_backbones_do():
    for name in MODULE_SHARED:
        assert getattr(ChannelMapper, name) is getattr(HipModule, name), name
        assert getattr(HipBackbone, name) is getattr(HipModule, name), name
    assert "train_form" not in ChannelMapper.__dict__ and HipModule.train_form == "torch"
    assert ResNetBackbone._run_backward is HipBackbone._run_backward
    assert ResNetBackbone.backward_struct is _hip.BackboneBwdOpStruct and ResNetBackbone.backward_prefix == "sdetr_backbone_bwd"


def test_one_autograd_node_serves_every_forward_hip_train():
    """Source level: the modules with a ``forward_hip_train`` define one ``torch.autograd.Function`` subclass between them."""
    files = ("hip_module", "backbone_base", "channel_mapper", "backbone", "convnext", "focalnet", "swin")
    found = []
    for name in files:
        with open(os.path.join(os.path.dirname(hip_module.__file__), name + ".py")) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef) and any(ast.unparse(b).endswith("autograd.Function") for b in node.bases):
                found.append(f"{name}.{node.name}")
    assert found == ["hip_module._TrainFunction"]


def _focalnet():
    return FocalNetBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,))


def _swin():
    return SwinBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,), num_heads=(2,), window_size=(7, 7))


def _no_library(*a, **k):
    raise AssertionError("the library was asked for")


@pytest.mark.parametrize("make", [_focalnet])
def test_a_backbone_without_a_hip_backward_refuses_the_hip_form(make, monkeypatch):
    m = make()
    assert m.hip_form() and any(p.requires_grad for p in m.parameters())
    assert m.train_form == "torch" and m.set_train_form("hip") is m and m.train_form == "hip"
    assert not m.hip_train_form() and "no HIP backward" in m.hip_train_reason()
    assert m.train_reasons is None and m.hip_train_reason() == "this backbone has no HIP backward"
    with pytest.raises(ValueError):
        m.set_train_form("triton")
    monkeypatch.setattr(_hip, "lib", _no_library)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no HIP backward"):
        m(x)
    outs = m.set_train_form("torch")(x)   # the composite, as before the switch existed
    assert all(t.requires_grad and not t.is_cuda for t in outs.values())


def test_swin_with_a_trainable_stem_refuses_the_hip_form_and_names_the_stem(monkeypatch):
    m = _swin()   # it has a HIP backward, but not of the stem, which freeze_indices=() leaves trainable
    assert m.hip_form() and any(p.requires_grad for p in m.body.features[0].parameters())
    assert m.train_form == "torch" and m.set_train_form("hip") is m and m.train_form == "hip"
    reason = m.hip_train_reason()
    assert not m.hip_train_form() and reason == SwinBackbone.train_reasons[1] != "this backbone has no HIP backward"
    assert "the stem (patch embedding and its LayerNorm, features.0) is trainable" in reason and "freeze_indices" in reason
    monkeypatch.setattr(_hip, "lib", _no_library)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError) as err:
        m(x)
    assert reason in str(err.value)
    outs = m.set_train_form("torch")(x)
    assert all(t.requires_grad and not t.is_cuda for t in outs.values())


# ------------------------------------------------------------------------------------------ the backward plan builder
SEQUENCE_SHARED = ("_trainable", "_first_trainable", "saved_activations", "stochastic_depth_factors", "_run_backward")


@pytest.mark.parametrize("cls", [ConvNeXtBackbone, SwinBackbone])
def test_the_backbones_that_walk_a_sequence_take_the_rest_from_the_base_too(cls):
    for name in SEQUENCE_SHARED:
        assert getattr(cls, name) is getattr(HipBackbone, name), name
    assert cls.backward_struct is getattr(_hip, {"ConvNeXtBackbone": "ConvnextBwdOpStruct", "SwinBackbone": "SwinBwdOpStruct"}[cls.__name__])
    assert cls.backward_prefix == {"ConvNeXtBackbone": "sdetr_convnext_bwd", "SwinBackbone": "sdetr_swin_bwd"}[cls.__name__]
    assert ResNetBackbone.saved_activations is not HipBackbone.saved_activations   # (a list, by op)


def _train_plans(case, monkeypatch):
    """The forward and backward plan of one training step of ``ct1`` / ``w7t`` on a zero CPU canvas, the two operand
    packers (the only library calls of plan building) replaced by stubs."""
    made = {}

    def packed(self, layer, layout=0, scale=None, scale_bias=True, pad_to=1):
        key = (layer, "packed", layout, scale is None, scale_bias, pad_to)
        return made.setdefault(key, (torch.zeros(8, dtype=torch.int16), torch.zeros(-(-layer.weight.shape[0] // pad_to) * pad_to)))

    def packed_rows_dgrad(self, layer, scale=None):
        return made.setdefault((layer, "dgrad", scale is None), torch.zeros(8, dtype=torch.int16))
    monkeypatch.setattr(HipBackbone, "_packed", packed)
    monkeypatch.setattr(HipBackbone, "_packed_rows_dgrad", packed_rows_dgrad)
    if case == "ct1":
        m = ConvNeXtBackbone(None, return_indices=CT.RETURN, freeze_indices=CT.FREEZE, stochastic_depth_prob=0.3,
                             block_setting=[CNBlockConfig(*r) for r in CT.setting(case)])
        x = torch.zeros(2, 3, 64, 96)
    else:
        m = SwinBackbone(None, return_indices=ST.RETURN, freeze_indices=ST.FREEZE, **ST.config(case, 0.2))
        x = torch.zeros(ST.CASES[case][1])
    m.train()
    train = {"first": m._first_trainable()}
    ops, outputs, keep, names = m.build_plan(x, 0, train)
    cots = {k: torch.zeros_like(v) for k, v in outputs.items()}
    bops, bnames, grads, bkeep = m._backward_ops(train["acts"], train["factors"], tuple(x.shape), cots)
    return m, (ops, names, keep), (bops, bnames, bkeep), grads, cots


def _pointers(op):
    return [getattr(op, f) for f, t in op._fields_ if t is ctypes.c_void_p and getattr(op, f) is not None]


# case -> (forward ops, backward ops, gradients, the rows op of two blocks of one stage and of a block of another)
PLANS = {"ct1": (26, 64, 53, ["features.5.0 (rows)", "features.5.1 (rows)", "features.3.1 (rows)"]),
         "w7t": (57, 101, 84, ["0.features.5.0.mlp.3 (rows)", "0.features.5.1.mlp.3 (rows)", "0.features.3.1.mlp.3 (rows)"])}


@pytest.mark.parametrize("case", list(PLANS))
def test_the_training_plans_build_on_the_cpu_and_point_into_what_they_keep(case, monkeypatch):
    m, fwd, bwd, grads, cots = _train_plans(case, monkeypatch)
    n_fwd, n_bwd, n_grads, rows = PLANS[case]
    assert (len(fwd[0]), len(bwd[0]), len(grads)) == (n_fwd, n_bwd, n_grads)
    assert len(fwd[1]) == n_fwd and len(bwd[1]) == n_bwd and len(set(bwd[1])) == n_bwd
    trainable = dict(m._trainable())
    assert set(grads) == set(trainable) and len(trainable) == n_grads
    for n, g in grads.items():
        assert g.shape == trainable[n].shape and g.dtype == torch.float32, n

    def spans(tensors):
        return sorted({(s.data_ptr(), s.data_ptr() + s.nbytes()) for s in (t.untyped_storage() for t in tensors)})
    # the backward also reads the forward's buffers (the stored activations, the factors)
    for (ops, names, _), held in ((fwd, spans(fwd[2])), (bwd, spans(list(bwd[2]) + list(fwd[2]) + list(cots.values())))):
        for op, name in zip(ops, names):
            for p in _pointers(op):
                assert any(a <= p < b for a, b in held), name
    written = spans(bwd[2])
    for n, g in grads.items():   # a gradient is a view of what the backward ops write
        assert any(a <= g.data_ptr() < b for a, b in written), n
    # scratch buffers are reused between the blocks of one stage (the plan runs in order on one stream)
    dzs = [bwd[0][bwd[1].index(r)].out for r in rows]
    assert dzs[0] == dzs[1] != dzs[2]


def test_resnet_load_weights_drops_num_batches_tracked_and_skips_a_mismatched_shape():
    torch.manual_seed(0)
    m = ResNetBackbone("resnet18")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    sd = {k: torch.randn_like(v) for k, v in before.items()}
    sd["bn1.num_batches_tracked"] = torch.tensor(7)
    sd["layer1.0.bn1.num_batches_tracked"] = torch.tensor(7)
    wrong = "layer2.0.conv1.weight"
    sd[wrong] = sd[wrong].reshape(-1)
    result = m.load_weights({"model": sd})
    assert list(result.unexpected_keys) == [] and list(result.missing_keys) == [wrong]
    after = m.state_dict()
    assert not any(k.endswith("num_batches_tracked") for k in after)
    for k, v in after.items():
        assert torch.equal(v, before[k] if k == wrong else sd[k]), k
