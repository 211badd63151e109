"""CPU: what the four backbones take from ``HipBackbone`` since the training interface moved there: the interface is
the base's own, a backbone without a HIP backward refuses the ``"hip"`` form with a reason instead of running something
else, and the ResNet loads checkpoints through the base's ``load_weights``."""
import pytest
import torch

from salience_detr_amd import _hip
from salience_detr_amd.backbone import ResNetBackbone
from salience_detr_amd.backbone_base import HipBackbone
from salience_detr_amd.convnext import ConvNeXtBackbone
from salience_detr_amd.focalnet import FocalNetBackbone
from salience_detr_amd.swin import SwinBackbone

SHARED = ("set_train_form", "hip_train_reason", "hip_train_form", "forward", "forward_hip_train", "_train_state",
          "load_weights")


@pytest.mark.parametrize("cls", [ResNetBackbone, ConvNeXtBackbone, FocalNetBackbone, SwinBackbone])
def test_the_training_interface_is_the_base_class_s(cls):
    for name in SHARED:
        assert getattr(cls, name) is getattr(HipBackbone, name), name
    assert "train_form" not in cls.__dict__ and HipBackbone.train_form == "torch"


def _focalnet():
    return FocalNetBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,))


def _swin():
    return SwinBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,), num_heads=(2,), window_size=(7, 7))


@pytest.mark.parametrize("make", [_focalnet, _swin])
def test_a_backbone_without_a_hip_backward_refuses_the_hip_form(make, monkeypatch):
    m = make()
    assert m.hip_form() and any(p.requires_grad for p in m.parameters())
    assert m.train_form == "torch" and m.set_train_form("hip") is m and m.train_form == "hip"
    assert not m.hip_train_form() and "no HIP backward" in m.hip_train_reason()
    with pytest.raises(ValueError):
        m.set_train_form("triton")

    def no_library(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_hip, "lib", no_library)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no HIP backward"):
        m(x)
    outs = m.set_train_form("torch")(x)   # the composite, as before the switch existed
    assert all(t.requires_grad and not t.is_cuda for t in outs.values())


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
