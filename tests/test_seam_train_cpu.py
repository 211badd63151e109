"""CPU: the reference of tests/seam_train_cases.py meets the conditions tests/test_seam_train_gpu.py relies on: the
float64 pair's gradients are finite and none is zero (a dropped term could not hide), the two yardsticks are finite and
ordered, and the fp32 CPU pair meets its own bar."""
import copy

import pytest
import torch

import seam_train_cases as S

GRAD_FLOOR = 5e-6   # as tests/test_frontend_train_gpu.py


@pytest.mark.parametrize("name", S.BACKBONES)
def test_float64_gradients_are_finite_and_none_is_zero(name):
    ref = S.reference(name)
    backbone = S.build_backbone(name)
    names = [n for n, _ in S.trainable(backbone, S.build_neck(backbone))] + S.seam_names()
    assert list(ref["g64"]) == names
    assert any(n.startswith("backbone.") for n in names) and any(n.startswith("neck.") for n in names)
    assert any(not p.requires_grad for p in backbone.parameters())       # freeze_indices took something out
    for n, g in ref["g64"].items():
        assert g.dtype == torch.float64 and torch.isfinite(g).all() and g.abs().max().item() > 0, n
    for l, (h, w) in enumerate(S.MAPS):
        assert tuple(ref["g64"][f"seam.{l}"].shape) == (S.CANVAS[0], backbone.num_channels[l], h, w)


@pytest.mark.parametrize("name", S.BACKBONES)
def test_yardsticks_are_finite_and_fp32_is_closer_than_bf16(name):
    ref = S.reference(name)
    for n in ref["g64"]:
        d32, dbf = ref["d32"][n], ref["dbf16"][n]
        assert 0 <= d32 < dbf < float("inf"), (n, d32, dbf)
        assert 0 <= ref["d32_norm"][n] < float("inf") and 0 <= ref["dbf16_norm"][n] < float("inf"), n
    print(name, "d32 %.2e .. %.2e, dbf16 %.2e .. %.2e" % (min(ref["d32"].values()), max(ref["d32"].values()),
                                                           min(ref["dbf16"].values()), max(ref["dbf16"].values())))


@pytest.mark.parametrize("name", S.BACKBONES)
def test_fp32_cpu_pair_meets_its_own_bar(name):
    ref = S.reference(name)
    for n, g64 in ref["g64"].items():
        own, norm = S.distance(ref["g32"][n], g64)
        bar = max(4 * ref["d32"][n], GRAD_FLOOR)
        assert own == ref["d32"][n] and own <= bar and norm <= bar, (n, own, norm, bar)


def test_the_reference_is_the_same_on_a_second_build():
    """Name-seeded weights, canvas and cotangents: a second pair gives the float64 gradients bit for bit."""
    backbone = S.build_backbone("swin")
    again = S.torch_grads(copy.deepcopy(backbone), S.build_neck(backbone), S.canvas(), S.cotangents())
    for n, g in S.reference("swin")["g64"].items():
        assert torch.equal(g, again[n]), n


def test_convnext_torch_form_hands_out_strided_maps():
    """Why the ChannelMapper takes strided inputs: the ConvNeXt composite's maps are channels-last in memory, the other
    three backbones' are contiguous.  (tests/test_seam_train_gpu.py builds its strided inputs itself.)"""
    contiguous = {}
    for name in S.BACKBONES:
        with torch.no_grad():
            maps = S.build_backbone(name).forward_torch(S.canvas())
        assert [tuple(m.shape[-2:]) for m in maps.values()] == S.MAPS, name
        contiguous[name] = [m.is_contiguous() for m in maps.values()]
    assert contiguous == {"resnet": [True] * 3, "convnext": [False] * 3, "swin": [True] * 3, "focalnet": [True] * 3}
