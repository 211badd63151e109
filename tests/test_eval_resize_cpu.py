"""CPU: ``EvalResize``'s host side -- the size rule against the reference's own shape arithmetic
(tests/golden/eval_resize_cases.npz, make_eval_resize_golden.py), the fixture's invariants the GPU test's exclusions rest
on, the new entry points' argument checks, and the detector's state dict with and without the resize."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eval_resize_cases as EC

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_resize_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def test_size_rule_equals_the_reference_on_every_stored_size(gold):
    from salience_detr_amd import eval_resize_size
    rows, out, differs = gold["size.rows"], gold["size.out"], gold["size.differs"]
    assert len(rows) >= 3000 and differs.sum() > 0          # the set where float32 and exact arithmetic disagree
    exact_wrong = 0
    for (h, w, mn, mx), want, diff in zip(rows.tolist(), out.tolist(), differs.tolist()):
        assert list(eval_resize_size(h, w, mn, mx)) == want, (h, w, mn, mx)
        exact_wrong += list(EC.exact_size(h, w, mn, mx)) != want
    assert exact_wrong == differs.sum()                      # (an exact rule fails on exactly those rows)
    for name, ((h, w), new, _) in EC.IMAGES.items():
        assert eval_resize_size(h, w, EC.MIN_SIZE, EC.MAX_SIZE) == new, name
    # the quirk at work: 3000 x 4000 under (800, 1333) is 799 x 1066 in the reference, not 800 x 1066
    assert eval_resize_size(480, 640, 800, 1333) == (800, 1066) and eval_resize_size(3000, 4000, 800, 1333) == (799, 1066)
    assert [3000, 4000, 800, 1333] in rows.tolist()


def _round64(gold, name):
    r = gold[f"{name}.u8.ref32"].copy().reshape(-1)
    r[gold[f"{name}.u8.diff_idx"]] = gold[f"{name}.u8.diff_val"]
    return r.reshape(gold[f"{name}.u8.ref32"].shape)


def test_fixture_invariants(gold):
    for name, ((h, w), (nh, nw), _) in EC.IMAGES.items():
        ref32 = gold[f"{name}.u8.ref32"]
        assert ref32.shape == (3, nh, nw) and gold[f"{name}.f32.ref64"].shape == (3, nh, nw)
        exc = np.unpackbits(gold[f"{name}.u8.excluded"])[:ref32.size].astype(bool)
        assert exc.mean() <= EC.EXCLUDED_CAP and abs(exc.mean() - gold[f"{name}.u8.share"]) < 1e-12
        # the reference's own uint8 output obeys the rule the GPU test applies: exact off the window, within 1 inside
        r64 = _round64(gold, name)
        differs = (r64 != ref32).reshape(-1)
        assert exc[differs].all() and np.abs(r64.astype(int) - ref32.astype(int)).max() <= 1
        d32, d8 = gold[f"{name}.f32.d_ref"], gold[f"{name}.u8.d_ref"]
        if (h, w) == (nh, nw):
            assert d32 == 0 and d8 == 0 and not exc.any()
            assert np.array_equal(gold[f"{name}.f32.ref64"], EC.image(name, "f32").numpy())
            assert np.array_equal(ref32, EC.image(name, "u8").numpy())
        else:
            assert 0 < d32 < 1e-5 and 0 < d8 < 2e-3
    assert tuple(gold["mixed.canvas_hw"]) == EC.MIXED_CANVAS
    assert gold["mixed.sizes"].tolist() == [list(EC.IMAGES[n][1]) for n in EC.MIXED]
    _, mask = EC.canvas64([gold[f"{n}.f32.ref64"] for n in EC.MIXED])
    assert np.array_equal(np.unpackbits(gold["mixed.mask"])[:mask.size].astype(bool), mask.reshape(-1))
    assert 0 < gold["mixed.u8.d_ref"] < 1e-5 and 0 < gold["mixed.f32.d_ref"] < 1e-4


def test_entry_points_reject_bad_arguments_without_gpu():
    from salience_detr_amd import _hip
    from salience_detr_amd.csrc import build
    build.build()
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        one = (ctypes.c_void_p * 1)(8)                       # non-null dummy: rejected before anything dereferences it
        hw, out_hw = (ctypes.c_int * 2)(4, 6), (ctypes.c_int * 2)(8, 12)
        f, g = lib.sdetr_backbone_resize_images, lib.sdetr_backbone_resize_batch_images
        assert f(None, None, hw, out_hw, 1, 0, one) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
        assert f(None, one, hw, out_hw, 1, 0, None) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
        assert f(None, one, hw, out_hw, 0, 0, one) == _hip.EINVAL and b"1 .. 64 images" in lib.sdetr_last_error()
        assert f(None, one, hw, out_hw, 65, 0, one) == _hip.EINVAL and b"1 .. 64 images" in lib.sdetr_last_error()
        assert f(None, one, hw, (ctypes.c_int * 2)(0, 12), 1, 1, one) == _hip.EINVAL and b"every side" in lib.sdetr_last_error()
        assert f(None, one, (ctypes.c_int * 2)(4, (1 << 24) + 1), out_hw, 1, 1, one) == _hip.EINVAL
        assert f(None, (ctypes.c_void_p * 1)(None), hw, out_hw, 1, 0, one) == _hip.EINVAL and b"image 0" in lib.sdetr_last_error()
        assert f(None, one, hw, out_hw, 1, 0, (ctypes.c_void_p * 1)(None)) == _hip.EINVAL and b"output 0" in lib.sdetr_last_error()
        assert g(None, one, hw, out_hw, 1, 0, 32, 32, None, 8) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
        assert g(None, one, hw, None, 1, 0, 32, 32, 8, 8) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
        assert g(None, one, hw, out_hw, 65, 0, 32, 32, 8, 8) == _hip.EINVAL and b"1 .. 64 images" in lib.sdetr_last_error()
        assert g(None, one, hw, out_hw, 1, 0, 32, 8, 8, 8) == _hip.EINVAL and b"does not fit" in lib.sdetr_last_error()
        assert g(None, one, hw, out_hw, 1, 0, 0, 32, 8, 8) == _hip.EINVAL and b"bad canvas" in lib.sdetr_last_error()


def test_host_side_refusals_need_no_gpu():
    from salience_detr_amd import EvalResize, batch_images
    from salience_detr_amd.eval_resize import InterpolationMode
    with pytest.raises(ValueError, match="no fallback"):
        EvalResize(64, 96, interpolation=InterpolationMode.BICUBIC)
    with pytest.raises(ValueError, match="no fallback"):
        EvalResize(64, 96, antialias=False)
    with pytest.raises(ValueError, match="no fallback"):
        EvalResize(64, 96, interpolation=3)
    with pytest.raises(ValueError):
        EvalResize(64.0, 96)
    r = EvalResize(64, 96, interpolation=2)
    assert (r.min_size, r.max_size) == (64, 96) and len(r.state_dict()) == 0 and r.output_size(301, 500) == (57, 96)
    img = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch_images([img], resize=(64, 96))
    with pytest.raises(ValueError, match="normalize=False"):
        batch_images([img], normalize=False, resize=(64, 96))


def _detector(**kw):
    from salience_detr_amd import SalienceDETR
    from salience_detr_amd.backbone import ResNetBackbone
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    return SalienceDETR(ResNetBackbone("resnet18", return_indices=(1, 2, 3)), ChannelMapper([128, 256, 512], 256, 4),
                        PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(50), **kw)


def test_detector_state_dict_and_modules_do_not_depend_on_the_resize():
    plain, sized = _detector(), _detector(min_size=800, max_size=1333)
    assert list(plain.state_dict()) == list(sized.state_dict())
    assert not hasattr(plain, "eval_resize")
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in sized.named_modules() if n != "eval_resize"]
    assert (sized.eval_resize.min_size, sized.eval_resize.max_size) == (800, 1333)
    # the reference's rule: the transform exists when at least one of the two is a number, with min(size), max(size)
    one = _detector(max_size=640)
    assert (one.eval_resize.min_size, one.eval_resize.max_size) == (640, 640)
    swapped = _detector(min_size=1333, max_size=800)
    assert (swapped.eval_resize.min_size, swapped.eval_resize.max_size) == (800, 1333)
