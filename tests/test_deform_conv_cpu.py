"""CPU: the deformable-conv composite (``salience_detr_amd/deform_conv.py``) against closed forms of ``F.conv2d`` in
float64, ``DeformConv2dPack``, the DCN ResNet's keys and the host side of its HIP form (form checks, the C entry's
validation).  torchvision is not a dependency: PyTorch's own conv is the judge."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import deform_conv_cases as DC
from salience_detr_amd import _hip
from salience_detr_amd.backbone import Bottleneck, ResNetBackbone
from salience_detr_amd.deform_conv import DeformConv2d, DeformConv2dPack, deform_conv2d

D = torch.float64
TOL = 1e-12


def _operands(k, groups=1, co=6, ci=4, h=9, w=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, ci, h, w, generator=g, dtype=D)
    wt = torch.randn(co, ci // groups, k, k, generator=g, dtype=D)
    b = torch.randn(co, generator=g, dtype=D)
    return x, wt, b


def _moved(x, dy, dx, p=1):
    """The zero-padded input translated by (dy, dx): a conv of it WITHOUT padding reads what the deformable taps read (a
    tap may move from the padding ring into the map, so the ring is part of the translated canvas)."""
    return DC.translate(F.pad(x, (p, p, p, p)), dy, dx)


def _zeros_offset(x, k, s, p, d, og=1):
    ho, wo = DC.out_hw(x.shape[2], k, s, p, d), DC.out_hw(x.shape[3], k, s, p, d)
    return torch.zeros(x.shape[0], 2 * og * k * k, ho, wo, dtype=D)


@pytest.mark.parametrize("k,s,d,groups", list(itertools.product((1, 3), (1, 2), (1, 2), (1, 2))))
def test_zero_offsets_and_unit_mask_are_the_plain_conv(k, s, d, groups):
    x, w, b = _operands(k, groups)
    p = d * (k - 1) // 2
    off = _zeros_offset(x, k, s, p, d)
    mask = torch.ones(2, k * k, *off.shape[2:], dtype=D)
    ref = F.conv2d(x, w, b, stride=s, padding=p, dilation=d, groups=groups)
    for m in (mask, None):
        got = deform_conv2d(x, off, w, b, stride=s, padding=p, dilation=d, mask=m)
        assert got.shape == ref.shape and (got - ref).abs().max().item() <= TOL


@pytest.mark.parametrize("dy,dx", [(1, 0), (0, -2), (3, 2), (-4, 5), (9, 0), (0, -11), (40, 40), (3e9, 0), (0, -3e9), (-3e9, 3e9)])
@pytest.mark.parametrize("s", [1, 2])
def test_constant_integer_offset_is_a_translation_with_zero_fill(dy, dx, s):
    x, w, b = _operands(3)
    off = _zeros_offset(x, 3, s, 1, 1)
    off[:, 0::2], off[:, 1::2] = dy, dx
    got = deform_conv2d(x, off, w, b, stride=s, padding=1)
    ref = F.conv2d(_moved(x, int(dy), int(dx)), w, b, stride=s)
    assert (got - ref).abs().max().item() <= TOL
    if abs(dy) >= 9 + 1 or abs(dx) >= 11 + 1:   # past the map and its padding ring: exactly the bias
        assert torch.equal(got, b.view(1, -1, 1, 1).expand_as(got))


@pytest.mark.parametrize("dy,dx", [(0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5)])
def test_half_pixel_offset_is_the_mean_of_two_translations(dy, dx):
    """The border rule: at dy = -0.5 the top row's tap ky = 1 samples y = -0.5, whose row -1 corner contributes zero --
    what the zero-filled translation says too."""
    x, w, b = _operands(3)
    off = _zeros_offset(x, 3, 1, 1, 1)
    off[:, 0::2], off[:, 1::2] = dy, dx
    got = deform_conv2d(x, off, w, b, padding=1)
    sy, sx = (1 if dy > 0 else -1) if dy else 0, (1 if dx > 0 else -1) if dx else 0
    ref = 0.5 * (F.conv2d(x, w, b, padding=1) + F.conv2d(_moved(x, sy, sx), w, b))
    assert (got - ref).abs().max().item() <= TOL
    top = 0.5 * F.conv2d(x, w[:, :, 1:2, 1:2].contiguous(), None)[:, :, 0]       # tap (1, 1) on row 0: half of row 0 alone
    if dy == -0.5:
        only = torch.zeros_like(w)
        only[:, :, 1, 1] = w[:, :, 1, 1]
        assert (deform_conv2d(x, off, only, None, padding=1)[:, :, 0] - top).abs().max().item() <= TOL


def test_single_tap_offsets_pin_the_channel_order():
    """dy on tap 2 alone and dx on tap 6 alone: each tap's weight slice on its own translated input plus the rest."""
    x, w, b = _operands(3)
    off = _zeros_offset(x, 3, 1, 1, 1)
    off[:, 2 * 2], off[:, 2 * 6 + 1] = 2.0, -3.0
    got = deform_conv2d(x, off, w, b, padding=1)

    def tap(t):
        only = torch.zeros_like(w)
        only[:, :, t // 3, t % 3] = w[:, :, t // 3, t % 3]
        return only
    rest = w - tap(2) - tap(6)
    ref = F.conv2d(x, rest, b, padding=1) + F.conv2d(_moved(x, 2, 0), tap(2), None) + F.conv2d(_moved(x, 0, -3), tap(6), None)
    assert (got - ref).abs().max().item() <= TOL


def test_mask_scales_the_output_and_each_tap():
    x, w, b = _operands(3, groups=2)
    off = _zeros_offset(x, 3, 1, 1, 1)
    plain = F.conv2d(x, w, None, padding=1, groups=2)
    quarter = torch.full((2, 9, 9, 11), 0.25, dtype=D)
    assert (deform_conv2d(x, off, w, None, padding=1, mask=quarter) - 0.25 * plain).abs().max().item() <= TOL
    per_tap = torch.linspace(0.1, 0.9, 9, dtype=D)
    mask = per_tap.view(1, 9, 1, 1).expand(2, 9, 9, 11).contiguous()
    ref = F.conv2d(x, w * per_tap.view(1, 1, 3, 3), None, padding=1, groups=2)
    assert (deform_conv2d(x, off, w, None, padding=1, mask=mask) - ref).abs().max().item() <= TOL


def test_offset_groups_sample_their_own_channels():
    x, w, b = _operands(3)
    off = _zeros_offset(x, 3, 1, 1, 1, og=2)
    off[:, 18 + 0::2][:, :9] = 1.0     # group 1 (channels 2..3): dy = 1 on every tap
    moved = torch.cat([_moved(x[:, :2], 0, 0), _moved(x[:, 2:], 1, 0)], 1)
    ref = F.conv2d(moved, w, b)
    assert (deform_conv2d(x, off, w, b, padding=1) - ref).abs().max().item() <= TOL


def test_gradcheck_float64():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 5, 6, generator=g, dtype=D, requires_grad=True)
    w = torch.randn(4, 2, 3, 3, generator=g, dtype=D, requires_grad=True)
    b = torch.randn(4, generator=g, dtype=D, requires_grad=True)
    # offsets away from integer positions (the bilinear kinks) by construction
    off = (torch.rand(2, 18, 3, 3, generator=g, dtype=D) * 0.6 + 0.2 + torch.randint(-2, 2, (2, 18, 3, 3), generator=g)
           ).requires_grad_(True)
    mask = torch.rand(2, 9, 3, 3, generator=g, dtype=D).requires_grad_(True)
    fn = lambda x, off, mask, w, b: deform_conv2d(x, off, w, b, stride=2, padding=1, mask=mask)
    assert torch.autograd.gradcheck(fn, (x, off, mask, w, b), eps=1e-6, atol=1e-6)


# ---- the pack and the DCN ResNet ------------------------------------------------------------------------------------

def test_fresh_pack_is_half_the_plain_conv():
    torch.manual_seed(0)
    pack = DeformConv2dPack(8, 6, 3, stride=2, padding=1, bias=False).double()
    assert list(dict(pack.named_children())) == ["conv_offset", "conv_mask", "deform_conv2d"]
    assert pack.conv_offset.out_channels == 18 and pack.conv_mask.out_channels == 9
    assert all(not p.any() for c in (pack.conv_offset, pack.conv_mask) for p in c.parameters())
    w = pack.deform_conv2d.weight
    assert w.abs().max().item() <= 1 / (8 * 9) ** 0.5 and isinstance(pack.deform_conv2d, DeformConv2d)
    x = torch.randn(2, 8, 7, 9, dtype=D)
    assert (pack(x) - 0.5 * F.conv2d(x, w, None, stride=2, padding=1)).abs().max().item() <= TOL


def _dcn(arch="resnet50", **kw):
    return ResNetBackbone(arch, stage_with_dcn=[False, True, True, True], **kw)


def test_dcn_resnet_keys_shapes_and_round_trip():
    """Raises NotImplementedError without the feature."""
    m = _dcn()
    sd = m.state_dict()
    widths = {2: 128, 3: 256, 4: 512}
    for stage, blocks in ((2, 4), (3, 6), (4, 3)):
        for j in range(blocks):
            p, c = f"layer{stage}.{j}.conv2.", widths[stage]
            assert tuple(sd[p + "conv_offset.weight"].shape) == (18, c, 3, 3) and tuple(sd[p + "conv_offset.bias"].shape) == (18,)
            assert tuple(sd[p + "conv_mask.weight"].shape) == (9, c, 3, 3) and tuple(sd[p + "conv_mask.bias"].shape) == (9,)
            assert tuple(sd[p + "deform_conv2d.weight"].shape) == (c, c, 3, 3)
            assert p + "deform_conv2d.bias" not in sd and p + "weight" not in sd
    assert "layer1.0.conv2.weight" in sd and not any(".conv_offset." in k for k in sd if k.startswith("layer1."))
    # what the reference's constructor leaves: its init loop re-draws every nn.Conv2d (the offset and mask convs too),
    # their biases stay zero, the deformable weight keeps the pack's uniform draw
    pack = m.layer2[0].conv2
    assert pack.conv_offset.weight.abs().max().item() > 0 and not pack.conv_offset.bias.any()
    assert pack.deform_conv2d.weight.abs().max().item() <= 1 / (128 * 9) ** 0.5
    other = _dcn()
    other.load_weights({"model": {k: v.clone() for k, v in sd.items()}})
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    assert list(other.state_dict()) == list(sd)


def test_dcn_composite_runs_and_trains_on_cpu():
    m = _dcn("resnet18", return_indices=(1,)).train()
    m.load_state_dict(DC.dcn_state(m, 3))
    out = m(torch.randn(1, 3, 32, 48))["layer2"]
    assert tuple(out.shape) == (1, 128, 4, 6)
    out.sum().backward()
    pack = m.layer2[1].conv2
    assert all(p.grad is not None and p.grad.abs().max().item() > 0 for p in pack.parameters())


def test_hip_form_of_dcn_archs():
    assert _dcn("resnet18").hip_form() and _dcn("resnet50").hip_form() and _dcn("wide_resnet50_2", return_indices=(1,)).hip_form()
    assert not _dcn("resnext50_32x4d").hip_form()
    assert not ResNetBackbone("resnet50", stage_with_dcn=[False, False, True, True],
                              replace_stride_with_dilation=[False, True, True]).hip_form()
    m = _dcn("resnet18", return_indices=(1,))
    m.layer2[0].conv2.deform_conv2d.bias = torch.nn.Parameter(torch.zeros(128))
    assert not m.hip_form()


def test_hip_train_reason_names_dcn():
    m = _dcn("resnet18", return_indices=(1, 2), freeze_indices=(0,))
    assert "DCN" in m.hip_train_reason()
    frozen = _dcn("resnet18", return_indices=(1, 2), freeze_indices=(0, 1, 2))
    assert frozen.hip_train_reason() is None
    late = ResNetBackbone("resnet18", stage_with_dcn=[False, True, False, False], return_indices=(1, 2), freeze_indices=(0, 1))
    assert late.hip_train_reason() is None     # the DCN stage is frozen with nothing trainable below it
    kinds = [d["conv"] for d in late.build_backward_plan(2, 64, 96)]
    assert kinds and not any(k.startswith("layer2.") and "conv" in k for k in kinds)
    through = ResNetBackbone("resnet18", stage_with_dcn=[False, False, True, False], return_indices=(1, 2), freeze_indices=(0,))
    for p in through.layer3.parameters():
        p.requires_grad = False
    assert "DCN" in through.hip_train_reason()   # layer2 is trainable below the frozen DCN stage: a dgrad through it


def test_c_entry_validates_the_deformable_op():
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        def op(**kw):
            f = dict(op=2, x=16, weight=16, bias=16, out=16, batch=2, in_channels=64, height=8, width=8, out_channels=64,
                     kernel_size=3, stride=1, padding=1, offset_mask=16)
            f.update(kw)
            return (_hip.BackboneOpStruct * 1)(_hip.BackboneOpStruct(**f))
        assert lib.sdetr_backbone_workspace_bytes(op(), 1, 0) == 0
        assert lib.sdetr_backbone_workspace_bytes(op(splits=4), 1, 1) == 0     # the reduction is never split
        assert lib.sdetr_backbone_conv_splits(op(splits=4), 0) == 1
        for bad, word in ((dict(offset_mask=None), "offset"), (dict(kernel_size=1, padding=0), "kernel 3"),
                          (dict(padding=0), "kernel 3"), (dict(in_channels=48), "in_channels"),
                          (dict(out_channels=60), "out_channels"), (dict(stride=3), "stride"), (dict(x_nchw=1), "x_nchw")):
            arr = op(**bad)
            assert lib.sdetr_backbone_workspace_bytes(arr, 1, 0) == -1, bad
            assert lib.sdetr_backbone_run(None, arr, 1, 0, None, 0) == -1
            assert word in lib.sdetr_last_error().decode(), (bad, lib.sdetr_last_error().decode())
        assert lib.sdetr_backbone_workspace_bytes(op(op=3, out_channels=32, offset_mask=None), 1, 1) >= 0
        assert lib.sdetr_backbone_workspace_bytes(op(op=3, out_channels=32, residual=16), 1, 1) == -1
        positional = _hip.BackboneOpStruct(0, 16, 16, 16, None, 16, None, 2, 64, 8, 8, 64, 3, 1, 1, 1, 0, 0)   # 18 values
        assert positional.offset_mask is None
