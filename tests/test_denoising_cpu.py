"""CPU: the host side of the denoising generator (``salience_detr_amd/denoising.py``) and of the detector's training
branch against the fixture made from the imported reference ``GenerateCDNQueries``
(tests/golden/make_denoising_golden.py): the group formula, the mask rule, the noise packing, the pure-torch restatement
the GPU tests use as their oracle, state-dict keys, argument rejection of the C entry points, no CPU fallback."""
import ctypes

import pytest
import torch

import denoising_cases as DC
from salience_detr_amd import _hip
from salience_detr_amd import denoising as D
from salience_detr_amd.set_criterion import dn_match_pattern

CASES = DC.load_cases()
TAGS = sorted(CASES)


def test_fixture_holds_the_cases_the_generator_is_specified_on():
    counts = {tuple(c.counts) for c in CASES.values()}
    assert {(3, 5), (0, 7), (1,), (0, 0), (100, 37), (130, 2)} <= counts
    assert any(c.p_label == 0 for c in CASES.values()) and any(c.s_box == 0 for c in CASES.values())
    main = CASES["main"]
    assert (main.C, main.E, main.groups, main.n_dn) == (91, 256, 20, 200)
    assert CASES["single"].groups == 100 and CASES["floor"].groups == 1
    assert CASES["over"].groups == 1 and CASES["over"].n_dn == 260
    clamp = CASES["clamp"]
    valid = clamp.noised_labels >= 0
    sig = clamp.box_queries.sigmoid()[valid]
    assert (clamp.box_queries[valid][:, 2:] < -6.9).sum() >= 2          # widths collapsed to 0 -> the eps clamp
    lo, hi = sig[:, :2] - sig[:, 2:] / 2, sig[:, :2] + sig[:, 2:] / 2
    assert (lo < 2e-3).sum() >= 2 and (hi > 1 - 2e-3).sum() >= 2        # boxes on the clamp at 0 and at 1
    for c in CASES.values():
        if c.flip is not None and c.flip.numel():
            assert ((c.flip - c.p_label * 0.5).abs() > 1e-6).all()


@pytest.mark.parametrize("tag", TAGS)
def test_group_formula(tag):
    c = CASES[tag]
    assert D.denoising_groups(c.nums, c.max_gt) == c.groups
    assert c.twice_max_gt == 2 * c.max_gt


@pytest.mark.parametrize("tag", TAGS)
def test_mask_rule(tag):
    c = CASES[tag]
    got = D.query_mask(c.max_gt, c.groups, c.Nq)
    assert got.dtype == torch.bool and got.shape == c.mask.shape
    assert torch.equal(got, c.mask)


@pytest.mark.parametrize("tag", TAGS)
def test_noise_packing_round_trips_the_recorded_draws(tag):
    c = CASES[tag]
    for cap in (max(c.max_gt, 1), c.max_gt + 5):
        noise = c.noise(cap)
        assert noise.shape == (2 * c.groups, len(c.counts) * cap, 10) and noise.dtype == torch.float32
        assert (noise >= 0).all() and (noise < 1).all()
        flip, new_label, sign, magnitude = D.unpack_noise(noise, c.counts, c.C)
        if c.flip is not None:
            assert torch.equal(flip, c.flip) and torch.equal(new_label, c.new_label.long())
        if c.sign is not None:
            assert torch.equal(sign, c.sign.float()) and torch.equal(magnitude, c.magnitude)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(tag):
    """The oracle of the GPU sweep, pinned to the reference's outputs: labels, masks and label rows exactly, boxes
    within the fp32 parity bar in inverse-sigmoid space and after the sigmoid the transformer applies."""
    c = CASES[tag]
    label_q, box_q, noised, mask = DC.restate_case(c, capacity=c.max_gt + 3)
    assert torch.equal(noised, c.noised_labels)
    assert torch.equal(mask, c.mask)
    assert torch.equal(label_q, c.expected_label_queries())
    if c.label_queries is not None:
        assert torch.equal(label_q, c.label_queries)
    assert box_q.shape == c.box_queries.shape
    if box_q.numel():
        err = (box_q - c.box_queries).abs().max().item()
        err_sig = (box_q.sigmoid() - c.box_queries.sigmoid()).abs().max().item()
        print(tag, "restatement box error", err, "after sigmoid", err_sig)
        assert err < DC.BOX_BAR and err_sig < DC.BOX_BAR
        pad = noised < 0
        assert (box_q[pad] == 0).all() and (label_q[pad] == 0).all()


@pytest.mark.parametrize("tag", TAGS)
def test_positive_slots_are_the_denoising_match(tag):
    c = CASES[tag]
    if c.n_dn == 0:
        return
    match = dn_match_pattern(c.counts, c.n_dn, c.groups, c.twice_max_gt)
    slot = torch.arange(c.n_dn)
    positive = (c.noised_labels >= 0) & ((slot // c.max_gt) % 2 == 0)[None]
    assert torch.equal(match >= 0, positive)
    t = (slot % c.max_gt).int()[None].expand_as(match)
    assert torch.equal(match[positive], t[positive])


def test_module_state_dict_and_constructor():
    gen = D.GenerateCDNQueries()
    assert (gen.num_queries, gen.num_classes, gen.label_embed_dim, gen.denoising_nums, gen.label_noise_prob,
            gen.box_noise_scale) == (300, 80, 256, 100, 0.5, 1.0)
    assert list(gen.state_dict()) == ["label_encoder.weight"]
    assert gen.label_encoder.weight.shape == (80, 256)
    gen = D.GenerateCDNQueries(900, 91, 32, 50, 0.3, 0.7)
    assert gen.label_encoder.weight.shape == (91, 32) and gen.denoising_nums == 50


def _head(**kw):
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETRHead
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer(embed_dim=32, num_heads=4, d_ffn=64, num_encoder_layers=2, num_decoder_layers=2,
                                    num_classes=7, topk_sa=6, two_stage_num_proposals=20)
    return SalienceDETRHead(ChannelMapper([16, 32], 32, 4), PositionEmbeddingSine(16, 10000, True, offset=-0.5), tr,
                            PostProcess(10), **kw)


def test_detector_state_dict_keys_with_and_without_criterion():
    from salience_detr_amd.detector import head_state_dict, train_state_dict
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion
    plain = _head()
    assert not any(k.startswith("denoising_generator") for k in plain.state_dict())
    assert not hasattr(plain, "denoising_generator")
    assert [n for n, _ in plain.named_children()] == ["neck", "position_embedding", "transformer", "postprocessor"]
    crit = HybridSetCriterion(7, HungarianMatcher(2, 5, 2), {"loss_class": 1.0})
    train = _head(criterion=crit, focus_criterion=SalienceCriterion(), num_classes=7, num_queries=20, denoising_nums=10)
    keys = set(train.state_dict())
    assert keys == set(plain.state_dict()) | {"denoising_generator.label_encoder.weight"}
    assert train.denoising_generator.label_encoder.weight.shape == (7, 32)
    assert (train.denoising_generator.num_queries, train.denoising_generator.denoising_nums) == (20, 10)
    # a reference-style state dict: every key of the training detector plus the class-name buffer
    full = {k: v.clone() for k, v in train.state_dict().items()}
    full["_classes_"] = torch.zeros(7, 8, dtype=torch.int64)
    train.load_state_dict(train_state_dict(full))
    plain.load_state_dict(head_state_dict(full))


def test_prepare_targets_converts_and_rejects_degenerate_boxes():
    from salience_detr_amd.detector import prepare_targets
    targets = [{"boxes": torch.tensor([[10.0, 20.0, 50.0, 100.0]]), "labels": torch.tensor([3])},
               {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}]
    out = prepare_targets(targets, [(200, 100), (64, 64)])
    assert torch.allclose(out[0]["boxes"], torch.tensor([[0.3, 0.3, 0.4, 0.4]]))
    assert targets[0]["boxes"][0, 0] == 10.0 and out[1]["boxes"].shape == (0, 4)
    assert out[0]["labels"] is targets[0]["labels"]
    with pytest.raises(RuntimeError, match="positive height and width"):
        prepare_targets([{"boxes": torch.tensor([[10.0, 20.0, 10.0, 100.0]]), "labels": torch.tensor([3])}], [(200, 100)])


def test_training_mode_needs_targets_and_a_criterion():
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion
    head = _head(criterion=HybridSetCriterion(7, HungarianMatcher(2, 5, 2), {"loss_class": 1.0}), num_classes=7,
                 num_queries=20)
    head.train()
    with pytest.raises(RuntimeError, match="needs targets"):
        head([torch.zeros(1, 16, 8, 8), torch.zeros(1, 32, 4, 4)], torch.zeros(1, 64, 64, dtype=torch.bool), [(64, 64)])
    with pytest.raises(RuntimeError, match="without a criterion"):
        _head().forward_train([], torch.zeros(1, 64, 64, dtype=torch.bool), [{}], [(64, 64)])


def test_entry_points_reject_bad_arguments_without_gpu():
    lib = _hip.lib()
    f = lib.sdetr_cdn_queries
    # stream, boxes, labels, offsets, capacity, weight, noise, B, max_gt, groups, C, E, Nq, p, s, outputs x 4
    def args(capacity=8, max_gt=5, groups=20, E=256, Nq=900, boxes=16, noise=16, out=16):
        return (None, boxes, 16, 16, capacity, 16, noise, 2, max_gt, groups, 91, E, Nq, 0.5, 1.0, out, 16, 16, 16)
    assert f(*args(boxes=None)) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert f(*args(out=None)) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert f(*args(noise=None)) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert f(*args(max_gt=9)) == _hip.EINVAL and b"max_gt" in lib.sdetr_last_error()
    assert f(*args(max_gt=0)) == _hip.EINVAL and b"max_gt" in lib.sdetr_last_error()
    assert f(*args(E=30)) == _hip.EINVAL and b"multiple of 4" in lib.sdetr_last_error()
    assert f(*args(groups=0)) == _hip.EINVAL and b"groups" in lib.sdetr_last_error()
    assert f(*args(Nq=2 ** 31 - 1)) == _hip.EINVAL and b"overflows" in lib.sdetr_last_error()
    assert f(*args(capacity=2 ** 20, max_gt=2 ** 20, groups=2 ** 10)) == _hip.EINVAL and b"overflows" in lib.sdetr_last_error()
    assert f(*args(boxes=8)) == _hip.EINVAL and b"aligned" in lib.sdetr_last_error()
    g = lib.sdetr_cdn_label_grad
    assert g(None, None, 16, 2, 200, 91, 256, 16) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert g(None, 16, 16, 2, 200, 91, 256, None) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert g(None, 16, 16, 2, 0, 91, 256, 16) == _hip.EINVAL and b"bad sizes" in lib.sdetr_last_error()
    assert g(None, 16, 16, 2 ** 20, 2 ** 20, 91, 256, 16) == _hip.EINVAL and b"overflows" in lib.sdetr_last_error()
    # the batching launch's new switch is checked like the old entry
    h = lib.sdetr_backbone_batch_images_ex
    assert h(None, None, None, 1, 0, 0, 32, 32, None, None) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    ptrs, hw = (ctypes.c_void_p * 1)(16), (ctypes.c_int * 2)(40, 8)
    assert h(None, ptrs, hw, 1, 0, 0, 32, 32, 16, 16) == _hip.EINVAL and b"does not fit" in lib.sdetr_last_error()


def test_host_tensors_are_refused():
    gen = D.GenerateCDNQueries(20, 7, 32)
    t = DC.random_targets((2, 3), 7, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gen([x["labels"] for x in t], [x["boxes"] for x in t])
    from salience_detr_amd.backbone import batch_images
    with pytest.raises(RuntimeError):
        batch_images([torch.zeros(3, 8, 8)], normalize=False)
    with pytest.raises(RuntimeError, match="float32"):
        batch_images([torch.zeros(3, 8, 8, dtype=torch.uint8)], normalize=False)
