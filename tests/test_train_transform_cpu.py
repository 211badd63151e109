"""CPU: the host half of the training transform (salience_detr_amd/train_transform.py) against the imported reference's
transforms (tests/golden/train_transform_cases.npz, make_train_transform_golden.py): the size rule, the draws under equal
seeds, the boxes bit for bit, and the fixture's own fp32-against-float64 accounting that the GPU test's bound rests on."""
import random

import numpy as np
import pytest
import torch

import train_transform_cases as TC
from salience_detr_amd import TrainTransform, sample_params, shortest_size, transform_targets
from salience_detr_amd.eval_resize import eval_resize_size
from salience_detr_amd.train_transform import plan_stats


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


# ---- draws -----------------------------------------------------------------------------------------------------------

def test_shortest_size_is_the_references_double_rule(gold):
    rows, out, differs = gold["size.rows"], gold["size.out"], gold["size.differs_f32"]
    assert np.array_equal(rows, TC.shortest_size_rows())
    got = np.array([shortest_size(h, w, mn, mx or None) for h, w, mn, mx in rows.tolist()])
    assert np.array_equal(got, out)
    # the sweep holds sizes (h, w <= 2000) where EvalResize's float32 rule gives another size: the two are not one rule
    assert differs.sum() > 0 and (rows[differs, :2] <= 2000).all()
    f32 = np.array([eval_resize_size(h, w, mn, mx or None) for h, w, mn, mx in rows[differs].tolist()])
    assert (f32 != out[differs]).any(axis=1).all()
    with pytest.raises(ValueError, match="positive"):
        shortest_size(0, 5, 48)


@pytest.mark.parametrize("preset", ["detr", "multiscale", "hflip"])
def test_sample_params_draws_what_the_reference_draws(gold, preset):
    tf = getattr(TrainTransform, preset)()
    assert (tf.scales, tf.max_size) == ((None, None) if preset == "hflip" else (TC.SCALES, TC.MAX_SIZE))
    if preset == "detr":
        assert (tf.crop_scales, tf.crop_range, tf.p_flip, tf.sanitize) == (TC.CROP_SCALES, TC.CROP_RANGE, TC.P_FLIP, True)
    else:
        assert tf.crop_scales is None and not tf.sanitize
    plans = gold[f"draw.{preset}"]
    assert plans.shape == (len(TC.REAL_SIZES), len(TC.DRAW_SEEDS), 10)
    for a, (h, w) in enumerate(TC.REAL_SIZES):
        for b, seed in enumerate(TC.DRAW_SEEDS):
            torch.manual_seed(seed)
            random.seed(seed)
            p = tf.sample(h, w)
            assert p.plan() == plans[a, b].tolist(), (preset, h, w, seed)
            if preset == "detr" and b == 0:      # the keyword form with the defaults is the same draw
                torch.manual_seed(seed)
                random.seed(seed)
                assert sample_params(h, w) == p
    if preset == "detr":     # both branches and both flips occur
        assert set(plans[..., 1].reshape(-1).tolist()) == {1, 2} and set(plans[..., 0].reshape(-1).tolist()) == {0, 1}


def test_forced_branches_take_no_choice_draw():
    for branch, stages in ((0, 1), (1, 2)):
        torch.manual_seed(3)
        random.seed(3)
        p = sample_params(480, 640, branch=branch)
        assert p.n_stages == stages
        # the same stream with the choice's draw removed by hand
        torch.manual_seed(3)
        random.seed(3)
        flip = bool(torch.rand(1) < 0.5)
        first = int(torch.randint(3 if branch else 11, ()))
        assert p.flip == flip
        if branch:
            assert p.size1 == shortest_size(480, 640, TC.CROP_SCALES[first])
        else:
            assert p.size == shortest_size(480, 640, TC.SCALES[first], TC.MAX_SIZE)


# ---- boxes and labels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(TC.BOX_CASES))
def test_transform_targets_bit_for_bit(gold, name):
    hw, plan, boxes = TC.BOX_CASES[name]
    extra = torch.tensor([7, 8, 9])
    target = {"boxes": TC.box_tensor(boxes), "labels": torch.arange(1, len(boxes) + 1), "image_id": extra, "note": "kept"}
    before = target["boxes"].clone()
    out = transform_targets(target, TC.params_from_plan(plan), *hw)
    want_b, want_l = gold[f"box.{name}.out"], gold[f"box.{name}.labels"]
    assert out["boxes"].dtype == torch.float32 and tuple(out["boxes"].shape) == want_b.shape
    assert np.array_equal(out["boxes"].numpy().view(np.uint32), want_b.view(np.uint32))        # bit for bit
    assert np.array_equal(out["labels"].numpy(), want_l)
    assert out["image_id"] is extra and out["note"] == "kept" and set(out) == set(target)
    assert torch.equal(target["boxes"], before) and len(target["labels"]) == len(boxes)       # the input is untouched
    if name == "empty":
        assert tuple(out["boxes"].shape) == (0, 4) and out["labels"].numel() == 0
    if name == "under_1px":
        assert want_l.tolist() == [2]
    if name == "on_border":
        assert want_l.tolist() == [1, 3, 4]


def test_presets_without_sanitize_do_not_filter():
    hw, plan, boxes = TC.BOX_CASES["under_1px"]
    target = {"boxes": TC.box_tensor(boxes), "labels": torch.tensor([1, 2])}
    out = transform_targets(target, TC.params_from_plan(plan), *hw, sanitize=False)
    assert out["boxes"].shape[0] == 2 and out["labels"] is target["labels"]
    kept = transform_targets(target, TC.params_from_plan(plan), *hw)
    assert torch.equal(out["boxes"][1:], kept["boxes"])
    same = transform_targets(target, TC.params_from_plan((0, 0, 0, 0, 0, 0, 0, 0) + hw), *hw, sanitize=False)
    assert torch.equal(same["boxes"], target["boxes"]) and same["boxes"] is not target["boxes"]
    with pytest.raises(RuntimeError, match=r"float32 \[n, 4\]"):
        transform_targets({"boxes": torch.zeros(2, 4, dtype=torch.float64)}, TC.params_from_plan(plan), *hw)


@pytest.mark.parametrize("case", TC.SEEDED, ids=lambda c: TC.seeded_name(*c))
def test_seeded_targets_equal_the_references_compose(gold, case):
    preset, hw, seed = case
    key = TC.seeded_name(*case)
    consts = dict(TC.SMALL)
    if preset != "detr":
        consts.update(crop_scales=None, crop_range=None, sanitize=False, flip_last=preset == "multiscale")
    if preset == "hflip":
        consts.update(scales=None, max_size=None)
    tf = TrainTransform(**consts)
    torch.manual_seed(seed)
    random.seed(seed)
    p = tf.sample(*hw)
    assert p.plan() == gold[f"{key}.plan"].tolist()
    out = transform_targets(TC.seeded_target(*case), p, *hw, sanitize=tf.sanitize)
    assert np.array_equal(out["boxes"].numpy().view(np.uint32), gold[f"{key}.boxes"].view(np.uint32))
    assert np.array_equal(out["labels"].numpy(), gold[f"{key}.labels"])


# ---- the fixture's own accounting ----------------------------------------------------------------------------------------

def test_fixture_fp32_and_float64_chains_agree_within_the_cap(gold):
    keys = [f"img.{n}.u8" for n in TC.IMAGE_CASES] + [TC.seeded_name(*c) for c in TC.SEEDED]
    total = differing = 0
    for key in keys:
        ref = gold[f"{key}.ref"].astype(np.int64).reshape(-1)
        idx, val = gold[f"{key}.diff_idx"], gold[f"{key}.diff_val"].astype(np.int64)
        share = len(idx) / ref.size
        assert share == float(gold[f"{key}.share"]) and share <= TC.SELF_SHARE, (key, share)
        assert len(idx) == 0 or (np.abs(ref[idx] - val) <= TC.SELF_STEP).all() and (ref[idx] != val).all(), key
        total += ref.size
        differing += len(idx)
    print(f"fp32 against float64 over {len(keys)} chains: {differing / total:.4%} of {total} values")
    assert 4 * TC.SELF_SHARE == TC.GPU_SHARE
    # the reference's ConvertImageDtype multiplies by fp32(1 / 255), csrc/image_norm.h divides by 255: a rounding apart
    assert 0 < float(gold["norm_gap"]) <= 1e-6


def test_the_presets_whole_range_stages():
    """Every second resize the ``detr`` preset can draw (a crop of 384 .. 600 per side to a shorter side of 480 .. 800) keeps
    its window in LDS: the extremes of the scale and of the aspect ratio, host arithmetic only."""
    worst = []
    for ch, cw in ((600, 600), (600, 384), (384, 600), (599, 463), (384, 384), (480, 599)):
        for scale in (480, 800):
            nh, nw = shortest_size(ch, cw, scale, 1333)
            p = TC.params_from_plan((0, 2, 640, 853, 0, 0, ch, cw, nh, nw))
            staged, recomputed = plan_stats([(480, 640)], [p])
            worst.append((ch, cw, nh, nw, staged, recomputed))
            assert recomputed == 0 and staged == -(-nh // 4) * -(-nw // 64), worst[-1]
    print("two-stage workgroups (crop h, w, out h, w, staged, recomputed):", worst)


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TrainTransform.detr()([torch.zeros(3, 40, 50, dtype=torch.uint8)], None)
