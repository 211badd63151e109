"""GPU: the pyramid flatten folded into the hoisted stage-1 launch of the salience head
(include/salience_hip.h, sdetr_salience_head_hoist_pyramid_x3; csrc/salience_head_core.h, PYR form of stage1_x3_body).

The reference is the two-launch path that stays in the tree: ``pyramid_flatten`` followed by ``salience_head_hoist`` on
its ``enc_output`` input.  The arithmetic per token is the same, so every comparison is ``torch.equal`` -- no tolerance.

Shapes: batch 2, 256 channels, level widths and token counts that are no multiples of 32 (a 32-token tile straddles image
rows and level boundaries; the last levels have fewer than 32 tokens in all; one pyramid puts four levels inside one
tile), two images with different valid sizes (the padding mask and the border rule of ``keep`` both bite)."""
import math

import pytest
import torch

from salience_detr_amd import filter_ops as F
from salience_detr_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PYRAMIDS = {
    "rows13": [(13, 17), (7, 9), (4, 5), (2, 3)],
    "rows5": [(5, 37), (3, 19), (2, 10), (1, 5)],
    "four_in_a_tile": [(6, 11), (3, 5), (2, 3), (1, 2)],
    "one_level": [(9, 35)],
    "wide": [(3, 67), (2, 34), (1, 17), (1, 9)],                       # 67 valid columns: keep drops the first and the last
    "six_levels": [(4, 9), (3, 7), (2, 5), (2, 3), (1, 3), (1, 2)],     # box side 0.05 * 2^5 > 0.99: keep drops level 5
}
# a level of at least 33 400 tokens: the size at which the schedule-dependent corruption of stage 1's LayerNorm phase was
# seen (csrc/salience_head_core.h), followed by a level that shares the last tile with it
LARGE = [(167, 201), (5, 7)]


def _masks(shapes, fractions=((1.0, 1.0), (0.72, 0.61))):
    """[B,H,W] bool per level, True on padding: image b is valid on the top-left ceil(fraction * size) rectangle."""
    out = []
    for h, w in shapes:
        m = torch.ones(len(fractions), h, w, dtype=torch.bool)
        for b, (fh, fw) in enumerate(fractions):
            vh, vw = max(1, math.ceil(fh * h)), max(1, math.ceil(fw * w))
            m[b, :vh, :vw] = False
        out.append(m)
    return out


def _predictor(seed):
    from salience_detr_amd.salience_filtering import MaskPredictor
    torch.manual_seed(seed)
    pred = MaskPredictor(256, 256).to(DEV)
    with torch.no_grad():
        pred.layer1[0].weight.add_((0.2 * syn.det_randn("s1f.g", (256,))).to(DEV))
    enc, norm = torch.nn.Linear(256, 256).to(DEV), torch.nn.LayerNorm(256).to(DEV)
    with torch.no_grad():
        enc.bias.add_((0.1 * syn.det_randn("s1f.eb", (256,))).to(DEV))
        norm.weight.add_((0.2 * syn.det_randn("s1f.ng", (256,))).to(DEV))
        norm.bias.add_((0.2 * syn.det_randn("s1f.nb", (256,))).to(DEV))
    return pred, enc, norm


def _case(name, shapes):
    B, C = 2, 256
    feats = [syn.det_randn(f"s1f.{name}.f{l}", (B, C, h, w)).to(DEV) for l, (h, w) in enumerate(shapes)]
    pos = [(0.7 * syn.det_randn(f"s1f.{name}.p{l}", (B, C, h, w))).to(DEV) for l, (h, w) in enumerate(shapes)]
    masks = [m.to(DEV) for m in _masks(shapes)]
    level_embeds = syn.det_randn(f"s1f.{name}.le", (len(shapes), C)).to(DEV)
    return feats, pos, masks, level_embeds


def _unfused(case, heads, act):
    feats, pos, masks, le = case
    pred, enc, norm = heads
    _, _, enc_in, mask, feat_act, pos_act, vr = F.pyramid_flatten(feats, pos, masks, le, want_bf16=act, want_fp32=False)
    mem = torch.zeros_like(enc_in)
    hh = F.salience_head_hoist(enc_in, pred, enc_output=enc, enc_output_norm=norm, memory_out=mem)
    return dict(feat=feat_act, pos=pos_act, mask=mask, valid_ratios=vr, g=hh.g, sigma=hh.sigma, memory=mem, c0=hh.c0,
                enc_in=enc_in)


def _fused(case, heads, act):
    feats, pos, masks, le = case
    pred, enc, norm = heads
    B, S = feats[0].shape[0], sum(f.shape[2] * f.shape[3] for f in feats)
    mem = torch.zeros((B, S, 256), device=DEV)
    hh, mask, feat_act, pos_act, vr = F.salience_head_hoist_pyramid(feats, pos, masks, le, pred, enc, norm, act, memory_out=mem)
    return dict(feat=feat_act, pos=pos_act, mask=mask, valid_ratios=vr, g=hh.g, sigma=hh.sigma, memory=mem, c0=hh.c0)


def _assert_same(a, b, what):
    assert set(a) - {"enc_in"} == set(b) - {"enc_in"}
    for k in set(a) - {"enc_in"}:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.fixture(scope="module")
def heads():
    return _predictor(11)


@pytest.mark.parametrize("act", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_fused_launch_gives_the_bits_of_flatten_then_stage1(name, act, heads):
    shapes = PYRAMIDS[name]
    case = _case(name, shapes)
    assert F.hoist_pyramid_applies(case[0], case[1], case[2], heads[0], heads[1], act)
    with torch.no_grad():
        ref = _unfused(case, heads, act)
        got = _fused(case, heads, act)
    # the cases do what they are for: padding and the keep border both occur, some levels are shorter than a tile
    assert ref["mask"].any() and not ref["mask"].all()
    assert (ref["valid_ratios"][1] < 1).any() and (ref["valid_ratios"][0] == 1).all()
    if name in ("wide", "six_levels"):   # ... and tokens that are no padding lose their row to the border / box-size rule
        assert ((ref["enc_in"] == 0).all(-1) & ~ref["mask"]).any()
    _assert_same(got, ref, name)


@pytest.mark.parametrize("name,shapes", list(PYRAMIDS.items()) + [("large", LARGE)])
def test_fused_launch_is_bit_reproducible(name, shapes, heads):
    case = _case(name, shapes)
    with torch.no_grad():
        first = _fused(case, heads, torch.bfloat16)
        if name == "large":
            assert shapes[0][0] * shapes[0][1] >= 33400
            _assert_same(first, _unfused(case, heads, torch.bfloat16), name)
        for i in range(4):
            _assert_same(_fused(case, heads, torch.bfloat16), first, (name, i))


def test_more_than_four_levels_in_a_tile_are_refused(heads):
    shapes = [(3, 3), (2, 2), (1, 3), (1, 2), (1, 1)]
    case = _case("five", shapes)
    assert not F.hoist_pyramid_applies(case[0], case[1], case[2], heads[0], heads[1], torch.bfloat16)
    with pytest.raises(RuntimeError):
        _fused(case, heads, torch.bfloat16)


def test_hot_path_takes_the_fused_launch_and_keeps_its_bits():
    """``SalienceEncoderHotPath.forward`` in the benchmark's mode (bf16 encoder, no aux outputs) with the flatten inside
    stage 1 and with the flatten's own launch: the same memory and salience scores, bit for bit."""
    from salience_detr_amd.hot_path import build_hot_path
    shapes = [(40, 61), (20, 31), (10, 16), (5, 8)]
    m = build_hot_path()
    m.load_state_dict(syn.det_state_dict(m.state_dict()))
    m = m.to(DEV).eval()
    m.set_encoder_dtype(torch.bfloat16, torch.float16)
    feats, pos, masks, _ = _case("hot", shapes)
    calls = []
    real = F.salience_head_hoist_pyramid
    try:
        F.salience_head_hoist_pyramid = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        with torch.no_grad():
            memory, scores = m(feats, masks, pos)
            assert calls == [1]
            F.FLATTEN_IN_STAGE1 = False
            memory2, scores2 = m(feats, masks, pos)
            assert calls == [1]
    finally:
        F.FLATTEN_IN_STAGE1 = True
        F.salience_head_hoist_pyramid = real
    assert torch.equal(memory, memory2)
    for a, b in zip(scores, scores2):
        assert torch.equal(a, b)
