"""CPU: the fixtures of the reference detector's training step (tests/golden/detector_train_<tag>.npz, made by
tests/golden/make_detector_train_golden.py) hold what tests/test_detector_train_gpu.py reads from them, and the host
side of this project agrees with them: the state-dict keys and name-seeded weights, the noise packing of the recorded
draws, target preparation, the group formula and the denoising match."""
import numpy as np
import pytest
import torch

import detector_train_cases as DT
from salience_detr_amd import denoising as D
from salience_detr_amd.detector import prepare_targets
from salience_detr_amd.set_criterion import dn_match_pattern

CASES = {tag: DT.Case(tag) for tag in DT.TAGS}


def test_fixtures_hold_the_three_target_layouts():
    assert CASES["small"].counts == [3, 2] and CASES["small"].groups == 4
    assert CASES["empty_first"].counts == [0, 4] and CASES["empty_first"].groups == 3
    one = CASES["groups_one"]
    assert one.counts == [5, 1] and one.denoising_nums < one.max_gt and one.groups == 1
    for c in CASES.values():
        assert c.sizes == DT.SIZES and int(c.d["groups"]) == c.groups
        assert set(c.losses) == set(DT.weight_dict())
        assert all(np.isfinite(v) and v > 0 for v in c.losses.values())
        # the float64 step's losses lie within fp32 rounding of the fp32 step's
        assert np.abs(c.d["loss_values64"] - c.d["loss_values"]).max() < 1e-5 * np.abs(c.d["loss_values"]).max()


@pytest.mark.parametrize("tag", DT.TAGS)
def test_detector_takes_the_reference_weights(tag):
    """``Case.detector`` checks the fixture's key list and checksums against ``synthetic.det_state_dict``; every
    parameter of the detector then is one the fixture has a gradient norm for, and the other way round."""
    c = CASES[tag]
    det = c.detector(c.stored_maps())
    own = dict(det.named_parameters(remove_duplicate=False))
    every = c.d["norm_names"].tolist()
    assert len(every) == len(set(every)) == 150
    assert set(every) == {n for n, _ in det.named_parameters()}
    stored = c.d["grad_names"].tolist()
    assert len(stored) == len(set(stored)) and stored[:3] == ["map0", "map1", "map2"]
    assert set(stored[3:]) <= set(own)
    shapes = {n: tuple(p.shape) for n, p in own.items()}
    shapes.update({f"map{i}": tuple(m.shape) for i, m in enumerate(c.stored_maps())})
    for n in stored:
        assert c.d[f"grad.{n}"].shape == tuple(c.stored(torch.empty(shapes[n])).shape), n


@pytest.mark.parametrize("tag", DT.TAGS)
def test_stored_gradients_are_finite_and_consistent(tag):
    d = CASES[tag].d
    stored = d["grad_names"].tolist()
    assert len(d["grad_max"]) == len(d["grad_d_ref"]) == len(stored)
    for n, m, d_ref in zip(stored, d["grad_max"].tolist(), d["grad_d_ref"].tolist()):
        g = d[f"grad.{n}"]
        assert g.dtype == np.float32 and np.isfinite(g).all(), n
        assert m > 0 and abs(np.abs(g).max() - m) <= 1e-6 * m, n        # stored as the float32 of a float64 value
        assert 0 <= d_ref < 2e-3 * 4, n     # the reference's own fp32 step lies within the standing bar of its float64 one
    norms, d_norm = d["grad_norms"], d["norm_d_ref"]
    assert norms.shape == d_norm.shape == (150,) and np.isfinite(norms).all() and (norms > 0).all()
    assert (d_norm >= 0).all() and d_norm.max() < 2e-3 * 4
    # a parameter stored in full: its norm in the digest is the norm of the stored tensor
    at = d["norm_names"].tolist().index("transformer.alpha")
    assert abs(np.linalg.norm(d["grad.transformer.alpha"].astype(np.float64)) - norms[at]) < 1e-6 * norms[at]
    # the spread reaches every part the training branch wires together
    for part in ("denoising_generator.", "neck.convs.3.0.", "transformer.alpha", "transformer.enc_mask_predictor.",
                 "transformer.encoder.layers.0.", "transformer.encoder.layers.1.", "transformer.decoder.layers.0.",
                 "transformer.decoder.layers.1.", "transformer.decoder.class_head.1.", "transformer.encoder_class_head.",
                 "transformer.decoder.bbox_head.0.", "transformer.decoder.ref_point_head."):
        assert any(n.startswith(part) for n in stored), part


@pytest.mark.parametrize("tag", DT.TAGS)
def test_recorded_draws_pack_and_targets_prepare(tag):
    c = CASES[tag]
    d = c.d
    noise = c.noise()
    assert noise.shape == (2 * c.groups, len(c.counts) * c.max_gt, 10) and noise.dtype == torch.float32
    flip, new_label, sign, magnitude = D.unpack_noise(noise, c.counts, DT.C)
    assert torch.equal(flip, torch.from_numpy(d["draw_flip"]))
    assert torch.equal(new_label, torch.from_numpy(d["draw_label"]).long())
    assert torch.equal(sign, torch.from_numpy(d["draw_sign"]).float().reshape(-1, 4))
    assert torch.equal(magnitude, torch.from_numpy(d["draw_magnitude"]).reshape(-1, 4))
    assert ((flip - 0.25).abs() > 1e-6).all()
    targets = c.targets()
    assert [t["boxes"].shape[0] for t in targets] == c.counts == [t["labels"].shape[0] for t in targets]
    prepared = prepare_targets(targets, c.sizes)
    for t in prepared:
        assert (t["boxes"] > 0).all() and (t["boxes"] < 1).all()
        assert ((t["labels"] >= 0) & (t["labels"] < DT.C)).all()
    n_dn = 2 * c.groups * c.max_gt
    match = dn_match_pattern(c.counts, n_dn, c.groups, 2 * c.max_gt)
    assert match.shape == (len(c.counts), n_dn)
    assert [(row >= 0).sum().item() for row in match] == [c.groups * n for n in c.counts]
