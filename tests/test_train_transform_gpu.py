"""GPU: the training transform in HIP (csrc/train_transform.hip, salience_detr_amd/train_transform.py).

Fused = composed is the strong pin: the one launch must equal, bit for bit, ``batch_images`` of the images built step by
step with the launches that are already held to the reference (``img.flip(-1)``, ``resize_images``, the slice,
``resize_images``).

Against the reference's fixture (tests/golden/train_transform_cases.npz: the reference's transform classes on tensors).
uint8: the canvas un-normalised back to 0..255 steps may differ from the reference on at most 1 % of a case's pixels and
nowhere by more than 2 steps -- one step from a rounding boundary in the intermediate image, one from a boundary in the
output; the fixture's own fp32-against-float64 disagreement is capped at a quarter of that share
(test_train_transform_cpu.py).  Float images: max abs error of the normalised canvas against the float64 chain at most
``max(4 d_ref, 2e-6 / min(std))``, the rule of test_eval_resize_gpu.py.  The mask and the padding are exact.  Every figure
is printed before it is asserted."""
import random

import numpy as np
import pytest
import torch

import train_transform_cases as TC
from salience_detr_amd import TrainTransform, batch_images
from salience_detr_amd.eval_resize import resize_images
from salience_detr_amd.train_transform import plan_stats

pytestmark = pytest.mark.gpu

# name -> ((h, w), plan).  Widths cross the 64-pixel tile, heights are no multiples of 4 (but where 5/4 exactly forces one).
COMPOSED = {
    "flip_only_odd":   ((37, 131), (1, 0, 0, 0, 0, 0, 0, 0, 37, 131)),
    "nothing":         ((37, 131), (0, 0, 0, 0, 0, 0, 0, 0, 37, 131)),
    "up":              ((37, 53), (0, 1, 0, 0, 0, 0, 0, 0, 75, 107)),
    "up_flip":         ((37, 53), (1, 1, 0, 0, 0, 0, 0, 0, 75, 107)),
    "down":            ((150, 201), (0, 1, 0, 0, 0, 0, 0, 0, 57, 77)),
    "down_flip":       ((150, 201), (1, 1, 0, 0, 0, 0, 0, 0, 57, 77)),
    "resize_flip":     ((61, 83), (2, 1, 0, 0, 0, 0, 0, 0, 54, 73)),
    "two_origin":      ((90, 130), (0, 2, 60, 86, 0, 0, 41, 70, 53, 91)),
    "two_corner":      ((90, 130), (1, 2, 60, 86, 15, 20, 45, 66, 59, 87)),
    "shrink_grow":     ((200, 290), (1, 2, 60, 87, 5, 7, 41, 66, 70, 113)),        # first resize: 3.3x, many taps
    "second_5_4":      ((100, 150), (0, 2, 80, 120, 3, 4, 61, 105, 49, 84)),       # 105 -> 84 is 5/4 exactly
    "second_5_4_both": ((100, 150), (1, 2, 80, 120, 3, 4, 65, 105, 52, 84)),       # both axes (the height is then 4 k)
    "second_8":        ((100, 600), (1, 2, 90, 560, 2, 3, 70, 528, 9, 66)),        # the recomputing path
    "crop_1x1":        ((40, 50), (0, 2, 30, 37, 11, 13, 1, 1, 5, 7)),
    "crop_1x1_wide":   ((40, 50), (1, 2, 30, 37, 29, 36, 1, 1, 6, 70)),
}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


def _image(name, hw, dtype):
    return TC.image(f"gpu.{name}", hw, "noise", dtype).cuda()


def composed(img, plan):
    """The image a plan gives, step by step with the launches already pinned to the reference."""
    flip, n, h1, w1, top, left, ch, cw, nh, nw = plan
    if flip == 1:
        img = img.flip(-1).contiguous()
    if n == 2:
        img = resize_images([img], [(h1, w1)])[0][:, top:top + ch, left:left + cw].contiguous()
    if n >= 1:
        img = resize_images([img], [(nh, nw)])[0]
    if flip == 2:
        img = img.flip(-1).contiguous()
    return img


def fused(imgs, plans, targets=None):
    return TrainTransform.detr()(imgs, targets, params=[TC.params_from_plan(p) for p in plans])


# ---- fused = composed --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TC.DTYPES)
@pytest.mark.parametrize("name", list(COMPOSED))
def test_fused_equals_composed_bit_for_bit(name, dtype):
    hw, plan = COMPOSED[name]
    img = _image(name, hw, dtype)
    batch = fused([img], [plan])
    want_c, want_m = batch_images([composed(img, plan)])
    assert batch.image_sizes == [tuple(plan[8:])] and batch.canvas.dtype == torch.float32 and batch.mask.dtype == torch.bool
    assert tuple(batch.canvas.shape) == tuple(want_c.shape)
    differing = int((batch.canvas != want_c).sum())
    staged, recomputed = plan_stats([hw], [TC.params_from_plan(plan)])
    print(f"{name} {dtype}: {hw} -> {tuple(plan[8:])}  canvas {tuple(want_c.shape)}  differing {differing}  "
          f"workgroups staged {staged} recomputed {recomputed}")
    assert torch.equal(batch.canvas, want_c) and torch.equal(batch.mask, want_m)
    if plan[1] != 2:
        assert (staged, recomputed) == (0, 0)
    elif name == "second_8":
        # every full tile reads 64 * 8 columns, far past the window; only the last corner tile (2 x 1 outputs at the
        # bottom-right border, where the taps are clipped) is small enough to stage: both paths run in one launch
        assert staged <= 1 and staged + recomputed == -(-plan[8] // 4) * -(-plan[9] // 64)
    else:
        assert recomputed == 0 and staged == -(-plan[8] // 4) * -(-plan[9] // 64)
    if plan[1] == 0:        # a bit-for-bit copy, mirrored or not
        src = img.flip(-1) if plan[0] else img
        assert torch.equal(batch.canvas, batch_images([src.contiguous()])[0])


# ---- against the reference's fixture -----------------------------------------------------------------------------------

def _check_u8(key, gold, canvas, mask):
    ref = gold[f"{key}.ref"].astype(np.int64)
    nh, nw = ref.shape[1:]
    c, m = canvas.cpu().numpy(), mask.cpu().numpy()
    assert not m[:nh, :nw].any() and m[nh:].all() and m[:, nw:].all()
    assert (c[:, nh:] == 0).all() and (c[:, :, nw:] == 0).all()
    off = np.abs(TC.unnormalize_to_steps(c, nh, nw) - ref)
    share = (off != 0).mean()
    print(f"{key}: {nh} x {nw}  pixels off the reference {share:.4%} (cap {TC.GPU_SHARE:.0%})  largest difference "
          f"{off.max()} (cap {TC.GPU_STEP})  the reference's own fp32 / float64 share {float(gold[f'{key}.share']):.4%}")
    assert share <= TC.GPU_SHARE and off.max() <= TC.GPU_STEP, key


@pytest.mark.parametrize("name", list(TC.IMAGE_CASES))
def test_uint8_images_against_the_reference(gold, name):
    hw, _, plan = TC.IMAGE_CASES[name]
    batch = fused([TC.case_image(name, "u8").cuda()], [plan])
    assert batch.image_sizes == [tuple(plan[8:])]
    _check_u8(f"img.{name}.u8", gold, batch.canvas[0], batch.mask[0])


@pytest.mark.parametrize("name", list(TC.IMAGE_CASES))
def test_float_images_within_the_references_own_error(gold, name):
    hw, _, plan = TC.IMAGE_CASES[name]
    batch = fused([TC.case_image(name, "f32").cuda()], [plan])
    ref = TC.normalize64(gold[f"img.{name}.f32.ref64"].astype(np.float64))
    nh, nw = ref.shape[1:]
    c, m = batch.canvas[0].cpu().numpy(), batch.mask[0].cpu().numpy()
    assert not m[:nh, :nw].any() and m[nh:].all() and m[:, nw:].all()
    assert (c[:, nh:] == 0).all() and (c[:, :, nw:] == 0).all()
    d_ref = float(gold[f"img.{name}.f32.d_ref"])
    err = np.abs(c[:, :nh, :nw].astype(np.float64) - ref).max()
    bound = max(4 * d_ref, 2e-6 / min(TC.STD))
    print(f"{name} f32: err {err:.3g}  d_ref {d_ref:.3g}  err / d_ref {err / d_ref if d_ref else 0:.3g}  bound {bound:.3g}")
    assert err <= bound, (name, err, bound)


# ---- a mixed batch -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TC.DTYPES)
def test_mixed_batch_equals_the_images_placed_in_a_canvas(dtype):
    names = ("flip_only_odd", "down_flip", "shrink_grow")          # no resize, one, two; three different sizes
    imgs = [_image(n, COMPOSED[n][0], dtype) for n in names]
    plans = [COMPOSED[n][1] for n in names]
    batch = fused(imgs, plans)
    sizes = [tuple(p[8:]) for p in plans]
    assert batch.image_sizes == sizes == [(37, 131), (57, 77), (70, 113)]
    assert tuple(batch.canvas.shape) == (3, 3, 96, 160) and tuple(batch.mask.shape) == (3, 96, 160)
    for b, (img, plan, (nh, nw)) in enumerate(zip(imgs, plans, sizes)):
        one = fused([img], [plan])
        assert torch.equal(batch.canvas[b, :, :nh, :nw], one.canvas[0, :, :nh, :nw])
        assert not batch.mask[b, :nh, :nw].any() and batch.mask[b, nh:].all() and batch.mask[b, :, nw:].all()
        assert (batch.canvas[b, :, nh:] == 0).all() and (batch.canvas[b, :, :, nw:] == 0).all()
    want_c, want_m = batch_images([composed(i, p) for i, p in zip(imgs, plans)])
    assert torch.equal(batch.canvas, want_c) and torch.equal(batch.mask, want_m)


# ---- seeded, end to end ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TC.SEEDED, ids=lambda c: TC.seeded_name(*c))
def test_seeded_end_to_end_reproduces_the_references_compose(gold, case):
    preset, hw, seed = case
    key = TC.seeded_name(*case)
    consts = dict(TC.SMALL)
    if preset != "detr":
        consts.update(crop_scales=None, crop_range=None, sanitize=False, flip_last=preset == "multiscale")
    if preset == "hflip":
        consts.update(scales=None, max_size=None)
    torch.manual_seed(seed)
    random.seed(seed)
    batch = TrainTransform(**consts)([TC.seeded_image(*case).cuda()], [TC.seeded_target(*case)])
    assert batch.image_sizes == [tuple(gold[f"{key}.plan"][8:].tolist())]
    assert np.array_equal(batch.targets[0]["boxes"].numpy().view(np.uint32), gold[f"{key}.boxes"].view(np.uint32))
    assert np.array_equal(batch.targets[0]["labels"].numpy(), gold[f"{key}.labels"])
    _check_u8(key, gold, batch.canvas[0], batch.mask[0])


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_errors_launch_nothing():
    u8, f32 = _image("err", (40, 50), "u8"), _image("err", (40, 50), "f32")
    ok = (0, 2, 30, 37, 1, 2, 20, 30, 24, 36)
    with pytest.raises(RuntimeError, match="does not lie inside the 30 x 37 intermediate"):
        fused([u8], [(0, 2, 30, 37, 11, 2, 20, 30, 24, 36)])
    with pytest.raises(RuntimeError, match="does not lie inside"):
        fused([u8], [(0, 2, 30, 37, 0, 8, 20, 30, 24, 36)])
    with pytest.raises(RuntimeError, match="n_stages must be 0, 1 or 2"):
        fused([u8], [(0, 3, 30, 37, 1, 2, 20, 30, 24, 36)])
    with pytest.raises(RuntimeError, match="n_stages 0 keeps the size"):
        fused([u8], [(0, 0, 0, 0, 0, 0, 0, 0, 24, 36)])
    with pytest.raises(ValueError, match="at most 64"):
        fused([u8] * 65, [ok] * 65)
    with pytest.raises(RuntimeError, match="one dtype"):
        fused([u8, f32], [ok] * 2)
    with pytest.raises(RuntimeError, match="float32 or uint8"):
        fused([f32.half()], [ok])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused([u8.cpu()], [ok])
    # a final size larger than the canvas: only the C entry can be handed one
    import ctypes
    from salience_detr_amd import _hip
    canvas, mask = torch.full((1, 3, 32, 32), 7.0, device="cuda"), torch.zeros(1, 32, 32, dtype=torch.bool, device="cuda")
    ptrs, hw = (ctypes.c_void_p * 1)(u8.data_ptr()), (ctypes.c_int * 2)(40, 50)
    with pytest.raises(RuntimeError, match="24 x 36 does not fit the 32 x 32 canvas"):
        _hip.launch("sdetr_backbone_train_batch_images", None, u8.device, ptrs, hw, (ctypes.c_int * 10)(*ok), 1, 1, 32, 32,
                    canvas.data_ptr(), mask.data_ptr())
    with pytest.raises(RuntimeError, match="null argument"):
        _hip.launch("sdetr_backbone_train_batch_images", None, u8.device, ptrs, hw, None, 1, 1, 32, 32,
                    canvas.data_ptr(), mask.data_ptr())
    torch.cuda.synchronize()
    assert (canvas == 7.0).all() and not mask.any()                  # nothing was launched
    batch = fused([u8] * 64, [ok] * 64)                               # 64 is served
    assert tuple(batch.canvas.shape) == (64, 3, 32, 64) and torch.equal(batch.canvas[0], batch.canvas[63])


# ---- the detector ------------------------------------------------------------------------------------------------------

def test_detector_forward_batch_equals_forward_on_the_cut_images():
    import detector_train_cases as DC
    case = DC.Case("small")
    assert case.sizes == [(64, 96), (48, 80)]
    det = case.detector([m.cuda() for m in case.stored_maps()]).cuda().train()
    noise = case.noise().cuda()
    raws = [(50, 70), (97, 131)]
    imgs = [_image(f"det{i}", hw, "u8") for i, hw in enumerate(raws)]
    plans = [(1, 2, 60, 84, 3, 5, 50, 75, 64, 96), (1, 1, 0, 0, 0, 0, 0, 0, 48, 80)]
    g = torch.Generator().manual_seed(5)
    targets = []
    for n, (h, w) in zip(case.counts, raws):
        x0, y0 = torch.rand(n, generator=g) * 0.3 * w + 0.3 * w, torch.rand(n, generator=g) * 0.3 * h + 0.3 * h
        targets.append({"boxes": torch.stack((x0, y0, x0 + 0.2 * w, y0 + 0.2 * h), -1),
                        "labels": torch.randint(0, DC.C, (n,), generator=g)})
    batch = fused(imgs, plans, targets)
    assert batch.image_sizes == case.sizes and [len(t["labels"]) for t in batch.targets] == case.counts
    got = det.forward_batch(batch, noise=noise)
    cut = [batch.canvas[b, :, :h, :w].contiguous() for b, (h, w) in enumerate(batch.image_sizes)]
    again_c, again_m = batch_images(cut, normalize=False)
    assert torch.equal(again_c, batch.canvas) and torch.equal(again_m, batch.mask)
    want = det(cut, batch.targets, noise=noise)
    torch.cuda.synchronize()
    assert set(got) == set(want) and len(got) > 0
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # the same refusals as the training forward
    with pytest.raises(RuntimeError, match="training mode needs targets"):
        det.forward_batch(batch._replace(targets=None))
    det.eval()
    with pytest.raises(RuntimeError, match="call train"):
        det.forward_batch(batch)
    det.train()
    crit, det.criterion = det.criterion, None
    with pytest.raises(RuntimeError, match="built without a criterion"):
        det.forward_batch(batch)
    det.criterion = crit
