"""CPU: the backbone's module surface (row N0): state-dict keys against the imported reference's
(tests/golden/backbone_cases.npz), checkpoint loading, the layer plan's shapes, argument checks of the HIP entries (no
launch), and the detector's state-dict helper."""
import os

import numpy as np
import pytest
import torch

import backbone_cases as BC
from salience_detr_amd import _hip
from salience_detr_amd.backbone import ResNetBackbone, plan_shapes

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_state_dict_keys_are_the_references(gold, name):
    arch, ret, _ = BC.CASES[name]
    m = ResNetBackbone(arch, return_indices=ret)
    assert list(m.state_dict()) == list(gold[f"{name}.keys"])
    assert m.num_channels == [64 * (4 if arch == "resnet50" else 1) * 2 ** i for i in ret]


def test_shallower_return_indices_drop_deeper_stages(gold):
    m = ResNetBackbone("resnet50", return_indices=(0, 1))
    keys = [k for k in gold["r50.keys"] if not k.startswith(("layer3.", "layer4."))]
    assert list(m.state_dict()) == keys and not hasattr(m, "layer3")


def test_torchvision_style_checkpoint_loads(tmp_path):
    m = ResNetBackbone("resnet18", return_indices=(1, 2, 3))
    sd = BC.syn.det_state_dict(m.state_dict(), salt=3)
    full = dict(sd)
    for k in list(sd):
        if k.endswith("running_var"):
            full[k.replace("running_var", "num_batches_tracked")] = torch.tensor(0)
    full["fc.weight"], full["fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    path = tmp_path / "r18.pth"
    torch.save({"model": full}, path)
    loaded = ResNetBackbone("resnet18", weights=str(path), return_indices=(1, 2, 3))
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(FileNotFoundError):
        ResNetBackbone("resnet18", weights=str(tmp_path / "missing.pth"))


def test_hip_form_and_dtypes():
    assert ResNetBackbone("resnet50").hip_form() and ResNetBackbone("resnet18").hip_form()
    assert ResNetBackbone("wide_resnet50_2", return_indices=(1,)).hip_form()
    assert not ResNetBackbone("resnext50_32x4d", return_indices=(1,)).hip_form()
    with pytest.raises(ValueError):
        ResNetBackbone("resnet50").set_dtype(torch.int32)
    with pytest.raises(ValueError):
        ResNetBackbone("resnet49")


@pytest.mark.parametrize("hw", [(64, 96), (97, 131), (33, 65), (800, 1344)])
def test_plan_shapes_follow_the_composite(hw):
    m = ResNetBackbone("resnet18", return_indices=(0, 1, 2, 3)).eval()
    shapes = plan_shapes(m.block, (2, 2, 2, 2), 4, *hw)
    if hw[0] * hw[1] > 20000:   # (the composite at full size is slow on a CPU: shapes only)
        assert shapes[-1][2:] == (25, 42)
        return
    with torch.no_grad():
        out = m.forward_torch(torch.zeros(1, 3, *hw))
    for name, c, h, w in shapes[2:]:
        assert tuple(out[name].shape) == (1, c, h, w)


def test_resnext_takes_the_composite_on_cpu():
    m = ResNetBackbone("resnext50_32x4d", return_indices=(0,)).eval()
    with torch.no_grad():
        out = m(torch.zeros(1, 3, 64, 64))
    assert tuple(out["layer1"].shape) == (1, 256, 16, 16)


def test_hip_form_on_cpu_tensor_raises():
    m = ResNetBackbone("resnet18", return_indices=(1,)).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))


def test_abi_entries_reject_bad_arguments():
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        assert lib.sdetr_backbone_packed_bytes(64, 3, 7, 0) == 3 * 64 * 160 * 2
        assert lib.sdetr_backbone_packed_bytes(64, 64, 3, 1) == 64 * 576 * 2
        assert lib.sdetr_backbone_packed_bytes(64, 64, 3, 2) == -1
        op = _hip.BackboneOpStruct(0, 16, 16, 16, None, 16, None, 2, 48, 8, 8, 64, 3, 1, 1, 1, 0, 0)
        arr = (_hip.BackboneOpStruct * 1)(op)
        assert lib.sdetr_backbone_workspace_bytes(arr, 1, 0) == -1      # 48 channels-last input channels
        assert lib.sdetr_backbone_conv_splits(arr, 0) == -1
        assert lib.sdetr_backbone_conv(None, arr, 0, None, 0) == -1
        assert "in_channels" in lib.sdetr_last_error().decode()
        arr[0].in_channels = 64
        assert lib.sdetr_backbone_conv(None, arr, 2, None, 0) == -1      # precision
        arr[0].op = 7
        assert lib.sdetr_backbone_run(None, arr, 1, 0, None, 0) == -1
        assert lib.sdetr_backbone_maxpool(None, None, 1, 8, 8, 64, 0, None) == -1
        assert lib.sdetr_backbone_batch_images(None, None, None, 1, 0, 32, 32, None, None) == -1


def test_detector_state_dict_helper():
    from salience_detr_amd.detector import detector_state_dict, head_state_dict
    sd = {"backbone.conv1.weight": torch.zeros(1), "neck.convs.0.0.weight": torch.zeros(1),
          "denoising_generator.label_encoder.weight": torch.zeros(1), "_classes_": torch.zeros(2)}
    assert list(detector_state_dict(sd)) == ["backbone.conv1.weight", "neck.convs.0.0.weight"]
    assert list(head_state_dict(sd)) == ["neck.convs.0.0.weight"]
