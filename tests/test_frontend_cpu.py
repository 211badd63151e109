"""CPU: the input stage's module boundary (row N7): state-dict keys and shapes equal the reference's
(tests/golden/frontend_cases.npz), constructor handling, which configurations take the HIP path, no CPU fallback."""
import math
import os
from functools import partial

import numpy as np
import pytest
import torch
from torch import nn

import frontend_cases as FC
from salience_detr_amd import _hip
from salience_detr_amd.channel_mapper import ChannelMapper
from salience_detr_amd.detector import SalienceDETRHead, head_state_dict
from salience_detr_amd.position_encoding import PositionEmbeddingSine, level_masks_and_positions

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


@pytest.mark.parametrize("name", list(FC.MAPPER_CASES))
def test_state_dict_keys_and_shapes_equal_reference(gold, name):
    cin, cout, num_outs, _, _ = FC.MAPPER_CASES[name]
    sd = ChannelMapper(list(cin), cout, num_outs).state_dict()
    assert list(sd.keys()) == list(gold[f"m.{name}.keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(gold[f"m.{name}.shapes"])


def test_constructor_arguments():
    m = ChannelMapper([64, 128], 64, 4)
    assert m.num_channels == [64] * 4
    assert [m.convs[i][0].kernel_size for i in range(4)] == [(1, 1)] * 2 + [(3, 3)] * 2
    assert [m.convs[i][0].stride for i in range(4)] == [(1, 1)] * 2 + [(2, 2)] * 2
    assert m.convs[2][0].in_channels == 128 and m.convs[3][0].in_channels == 64
    assert all(isinstance(m.convs[i][1], nn.GroupNorm) and m.convs[i][1].num_groups == 32 for i in range(4))
    assert all(m.convs[i][0].bias is None for i in range(4))
    # bias=None -> a conv bias only without a norm; an explicit bias is kept
    assert ChannelMapper([64], 64, 1, norm_layer=None).convs[0][0].bias is not None
    assert ChannelMapper([64], 64, 1, bias=True).convs[0][0].bias is not None
    act = ChannelMapper([64], 64, 1, activation_layer=nn.ReLU)
    assert isinstance(act.convs[0][2], nn.ReLU) and act.convs[0][2].inplace
    k3 = ChannelMapper([64], 64, 1, kernel_size=3)
    assert k3.convs[0][0].padding == (1, 1)


def test_init_weights_is_xavier():
    torch.manual_seed(0)
    m = ChannelMapper([512], 256, 2)
    w = m.convs[0][0].weight
    bound = math.sqrt(6.0 / (512 + 256))
    assert w.abs().max().item() <= bound and w.abs().max().item() > 0.9 * bound
    assert torch.equal(m.convs[0][1].weight, torch.ones(256))


def test_which_configurations_take_the_hip_path():
    assert ChannelMapper([512, 1024, 2048], 256, 4).hip_form()
    assert ChannelMapper([256, 512, 1024, 2048], 256, 4).hip_form()
    assert ChannelMapper([384, 768, 1536], 256, 6).hip_form()
    assert not ChannelMapper([512, 1000], 256, 3).hip_form()               # width not a multiple of 32
    assert not ChannelMapper([512], 256, 2, kernel_size=3).hip_form()
    assert not ChannelMapper([512], 256, 2, activation_layer=nn.ReLU).hip_form()
    assert not ChannelMapper([512], 256, 2, bias=True).hip_form()
    assert not ChannelMapper([512], 256, 2, norm_layer=partial(nn.BatchNorm2d)).hip_form()
    assert not ChannelMapper([512], 256, 2, groups=2).hip_form()
    assert not ChannelMapper([512], 256, 2, dilation=2).hip_form()
    # a second extra level reads out_channels channels: it too must be a multiple of 32
    assert ChannelMapper([64], 48, 2, norm_layer=partial(nn.GroupNorm, 16)).hip_form()
    assert not ChannelMapper([64], 48, 3, norm_layer=partial(nn.GroupNorm, 16)).hip_form()
    assert ChannelMapper([64], 64, 3).hip_form()


def test_training_form_is_the_torch_composite_on_cpu():
    """Grad enabled on parameters that require it: the differentiable composite, which equals the holders' own modules."""
    torch.manual_seed(0)
    m = ChannelMapper([64, 128], 64, 3)
    xs = [torch.randn(1, 64, 6, 7), torch.randn(1, 128, 3, 4)]
    outs = m({"a": xs[0], "b": xs[1]})
    want = m.convs[2](xs[1])
    assert torch.equal(outs[2], want) and outs[0].requires_grad


def test_no_cpu_fallback():
    m = ChannelMapper([64], 64, 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m([torch.zeros(1, 64, 4, 4)])
    pe = PositionEmbeddingSine(16, normalize=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pe(torch.zeros(1, 4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        level_masks_and_positions(torch.zeros(1, 8, 8, dtype=torch.bool), [(4, 4)], pe)


def test_position_buffers_and_set_dtype():
    pe = PositionEmbeddingSine(128, temperature=(10000, 20), normalize=True, offset=-0.5)
    dim_t = 2 * torch.arange(128).div(2, rounding_mode="floor") / 128
    assert torch.equal(pe.dim_tx, 10000 ** dim_t) and torch.equal(pe.dim_ty, 20 ** dim_t)
    assert set(pe.state_dict()) == {"dim_tx", "dim_ty"}
    m = ChannelMapper([64], 64, 1)
    assert m.set_dtype(torch.bfloat16).compute_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        m.set_dtype(torch.int32)


def test_head_state_dict_keys(gold):
    """A reference SalienceDETR state dict minus backbone.* / denoising_generator.* loads into the head: its neck and
    position keys are the reference mapper's and the sine module's, under the reference's attribute names."""
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer()
    head = SalienceDETRHead(ChannelMapper([512, 1024, 2048], 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                            tr, PostProcess(100))
    keys = list(head.state_dict().keys())
    ref_neck = ["neck." + k for k in gold["m.r50.keys"]]
    assert [k for k in keys if k.startswith("neck.")] == ref_neck
    assert [k for k in keys if k.startswith("position_embedding.")] == ["position_embedding.dim_tx",
                                                                        "position_embedding.dim_ty"]
    assert [k for k in keys if k.startswith("transformer.")] == ["transformer." + k for k in tr.state_dict()]
    full = dict(head.state_dict())
    full["backbone.body.conv1.weight"] = torch.zeros(1)
    full["denoising_generator.label_encoder.weight"] = torch.zeros(1)
    full["_classes_"] = torch.zeros(91, 8, dtype=torch.int64)   # registered by the reference's training script
    head.load_state_dict(head_state_dict(full))


def test_abi_symbols_present():
    lib = _hip.lib()
    for name in ("sdetr_frontend_conv", "sdetr_frontend_groupnorm", "sdetr_frontend_masks_positions",
                 "sdetr_frontend_workspace_bytes", "sdetr_frontend_conv_splits", "sdetr_frontend_pack_weight",
                 "sdetr_frontend_packed_bytes"):
        assert hasattr(lib, name)
    assert lib.sdetr_abi_version() == 1
    lvl = (_hip.FrontendLevelStruct * 1)(_hip.FrontendLevelStruct(None, None, 48, 4, 4, 1, None, None, None))
    assert lib.sdetr_frontend_workspace_bytes(lvl, 1, 1, 64) == -1          # 48 input channels: not a multiple of 32
    assert lib.sdetr_frontend_packed_bytes(100, 0) == 600 and lib.sdetr_frontend_packed_bytes(100, 1) == 200
    assert lib.sdetr_frontend_packed_bytes(100, 2) == -1
