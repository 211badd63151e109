"""GPU: ``EvalResize`` in HIP (csrc/eval_resize.hip) -- the resize-only launch and the launch fused with image batching
against the imported reference (tests/golden/eval_resize_cases.npz, make_eval_resize_golden.py), and the detector that
takes images of any size.

Bounds.  Float images: max abs error against the reference's float64 resize at most ``max(4 d_ref, 2e-6)``, ``d_ref`` being
the reference's own fp32 distance from float64 on that image (the factor 4 is the margin this suite gives a different
summation order over the same fp32 data, test_detector_train_gpu.py; the floor covers smooth images, where the
reference's sum happens to land within 1e-7: an fp32 sum of ~20 weighted taps at full scale 1 plus the weight
normalisation is good to about 1e-6 whatever its order; the fixture stores the float64 values as fp32, 3e-8).  uint8
images: with ``tau = max(4 d_ref, 1e-3)`` on the 0..255 scale, every pixel whose float64 value is at least ``tau`` from a
.5 boundary equals ``round_half_even`` of it exactly, the others (at most 2 % of an image, asserted on the fixture by
test_eval_resize_cpu.py) may differ by 1.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import eval_resize_cases as EC
from salience_detr_amd import EvalResize, batch_images, eval_resize_size, graph_guard
from salience_detr_amd.eval_resize import InterpolationMode, resize_images

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_resize_cases.npz")
MN, MX = EC.MIN_SIZE, EC.MAX_SIZE


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _round64(gold, name):
    r = gold[f"{name}.u8.ref32"].copy().reshape(-1)
    r[gold[f"{name}.u8.diff_idx"]] = gold[f"{name}.u8.diff_val"]
    return r.reshape(gold[f"{name}.u8.ref32"].shape)


def _excluded(gold, name):
    shape = gold[f"{name}.u8.ref32"].shape
    return np.unpackbits(gold[f"{name}.u8.excluded"])[:int(np.prod(shape))].astype(bool).reshape(shape)


# ---- 1, 2, 5: the resize-only launch against the reference -------------------------------------------------------------

@pytest.mark.parametrize("name", list(EC.IMAGES))
def test_float_images_within_the_references_own_error(gold, name):
    out = EvalResize(MN, MX)(EC.image(name, "f32").cuda())
    assert out.dtype == torch.float32 and tuple(out.shape) == (3,) + EC.IMAGES[name][1]
    ref, d_ref = gold[f"{name}.f32.ref64"].astype(np.float64), float(gold[f"{name}.f32.d_ref"])
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    bound = max(4 * d_ref, 2e-6)
    print(f"{name} f32: err {err:.3g}  d_ref {d_ref:.3g}  err / d_ref {err / d_ref if d_ref else 0:.3g}  bound {bound:.3g}")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name", list(EC.IMAGES))
def test_uint8_images_round_as_the_float64_statement(gold, name):
    out = EvalResize(MN, MX)(EC.image(name, "u8").cuda())
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3,) + EC.IMAGES[name][1]
    got, want, exc = out.cpu().numpy().astype(int), _round64(gold, name).astype(int), _excluded(gold, name)
    assert exc.mean() <= EC.EXCLUDED_CAP
    off = np.abs(got - want)
    print(f"{name} u8: excluded share {exc.mean():.4%}  pixels off by one {int((off == 1).sum())}  "
          f"outside the window {int((off[~exc] != 0).sum())}  largest difference {off.max()}")
    assert (off[~exc] == 0).all() and off.max() <= 1, name


# ---- 3: identity -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", EC.DTYPES)
def test_identity_size_is_a_copy(dtype):
    img = EC.image("identity", dtype).cuda()
    h, w = img.shape[1:]
    assert eval_resize_size(h, w, MN, MX) == (h, w)
    assert torch.equal(EvalResize(MN, MX)(img), img)
    canvas, mask = batch_images([img], resize=(MN, MX))
    want_c, want_m = batch_images([img])
    assert torch.equal(canvas, want_c) and torch.equal(mask, want_m)


# ---- 4, 5: fused = composed, and the canvas against the reference ----------------------------------------------------

@pytest.mark.parametrize("dtype", EC.DTYPES)
def test_fused_equals_composed_and_the_reference_canvas(gold, dtype):
    imgs = [EC.image(n, dtype).cuda() for n in EC.MIXED]
    canvas, mask = batch_images(imgs, resize=(MN, MX))
    resized = [EvalResize(MN, MX)(i) for i in imgs]
    assert [list(r.shape[1:]) for r in resized] == gold["mixed.sizes"].tolist()
    assert tuple(canvas.shape) == (3, 3) + tuple(gold["mixed.canvas_hw"]) and canvas.dtype == torch.float32
    want_c, want_m = batch_images(resized)
    assert torch.equal(canvas, want_c) and torch.equal(mask, want_m)
    one_launch = resize_images(imgs, [r.shape[1:] for r in resized])      # the batch through one resize-only launch
    assert all(torch.equal(a, b) for a, b in zip(one_launch, resized))
    # against the fixture
    if dtype == "f32":
        ref_c, ref_m = EC.canvas64([gold[f"{n}.f32.ref64"].astype(np.float64) for n in EC.MIXED])
    else:
        ref_c, ref_m = EC.canvas64([_round64(gold, n).astype(np.float64) / 255 for n in EC.MIXED])
    assert np.array_equal(mask.cpu().numpy(), ref_m)
    assert np.array_equal(np.unpackbits(gold["mixed.mask"])[:ref_m.size].astype(bool), ref_m.reshape(-1))
    err = np.abs(canvas.cpu().numpy().astype(np.float64) - ref_c)
    bound = max(4 * float(gold[f"mixed.{dtype}.d_ref"]), 2e-6 / min(EC.STD))
    if dtype == "u8":     # on the excluded pixels one uint8 step is allowed
        step = np.zeros_like(err)
        for b, n in enumerate(EC.MIXED):
            e = _excluded(gold, n)
            step[b, :, :e.shape[1], :e.shape[2]] = e / 255.0 / np.array(EC.STD).reshape(3, 1, 1)
        print(f"mixed u8: err off the window {err[step == 0].max():.3g}  bound {bound:.3g}  "
              f"pixels a step off {int((err > bound).sum())}")
        assert (err <= bound + step * (1 + 1e-6)).all()
    else:
        print(f"mixed f32: err {err.max():.3g}  d_ref {float(gold['mixed.f32.d_ref']):.3g}  bound {bound:.3g}")
        assert err.max() <= bound


# ---- 6: determinism and capture ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", EC.DTYPES)
def test_two_runs_and_graph_replay_bit_identical(dtype):
    imgs = [EC.image(n, dtype).cuda() for n in EC.MIXED]
    a = [t.clone() for t in batch_images(imgs, resize=(MN, MX))]
    b = batch_images(imgs, resize=(MN, MX))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        batch_images(imgs, resize=(MN, MX))
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = batch_images(imgs, resize=(MN, MX))
    torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    out[0].fill_(7.0)
    out[1].fill_(False)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a[0], out[0]) and torch.equal(a[1], out[1])


# ---- 7: the detector ---------------------------------------------------------------------------------------------------

def _detector(**kw):
    import backbone_cases as BC
    from salience_detr_amd.backbone import ResNetBackbone
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    det = SalienceDETR(ResNetBackbone("resnet50", return_indices=(1, 2, 3)), ChannelMapper([512, 1024, 2048], 256, 4),
                       PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(50), **kw)
    det.load_state_dict(BC.syn.det_state_dict(det.state_dict(), salt=5))
    return det.eval().cuda()


def test_detector_resizes_and_reports_boxes_in_original_pixels():
    from salience_detr_amd import synthetic as syn
    from salience_detr_amd.detector import SalienceDETRHead
    mn, mx = 160, 224
    raw = [(97, 131), (240, 300)]                       # one stretched, one shrunk
    imgs = [syn.det_rand(f"eval_resize.det{i}", (3, h, w)).cuda() for i, (h, w) in enumerate(raw)]
    new = [eval_resize_size(h, w, mn, mx) for h, w in raw]
    assert new == [(160, 216), (160, 200)]
    det = _detector(min_size=mn, max_size=mx)
    got = det(imgs)
    with torch.no_grad():
        canvas, mask = batch_images(imgs, resize=(mn, mx))
        want = SalienceDETRHead.forward(det, det.backbone(canvas), mask, torch.tensor(raw, device="cuda"),
                                        image_sizes=[list(s) for s in new], canvas=tuple(canvas.shape[-2:]))
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(g[k], w[k]), k
    # the same detector without the keywords on the pre-resized images: the same boxes in the resized pixels
    plain = _detector()
    assert list(plain.state_dict()) == list(det.state_dict())
    pre = plain([EvalResize(mn, mx)(i) for i in imgs])
    for g, p, (h, w), (nh, nw) in zip(got, pre, raw, new):
        assert torch.equal(g["scores"], p["scores"]) and torch.equal(g["labels"], p["labels"])
        factor = torch.tensor([w / nw, h / nh, w / nw, h / nh], device="cuda", dtype=torch.float64)
        want_boxes = p["boxes"].double() * factor
        tol = 4 * 2.0 ** -24 * max(h, w)                # a few fp32 roundings of a coordinate as large as the image
        err = (g["boxes"].double() - want_boxes).abs().max().item()
        print(f"boxes {h}x{w} <- {nh}x{nw}: err {err:.3g}  tol {tol:.3g}")
        assert err <= tol
        assert (g["boxes"] - p["boxes"]).abs().max().item() > 1.0       # (and they do differ)


class _StubBackbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.c2, self.c3, self.c4 = nn.Conv2d(3, 32, 8, 8), nn.Conv2d(32, 64, 2, 2), nn.Conv2d(64, 64, 2, 2)

    def forward(self, x):
        a = self.c2(x)
        b = self.c3(a.relu())
        return {"layer2": a, "layer3": b, "layer4": self.c4(b.relu())}


def _train_detector(**kw):
    from salience_detr_amd import synthetic as syn
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.salience_transformer import build_salience_transformer
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion
    classes, proposals, layers = 7, 10, 2
    base = {"loss_class": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    weights = dict(base)
    for suffix in ["_dn", "_enc"] + [f"_{i}" for i in range(layers - 1)] + [f"_dn_{i}" for i in range(layers - 1)]:
        weights.update({k + suffix: v for k, v in base.items()})
    weights["loss_salience"] = 2.0
    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2, num_decoder_layers=layers,
                                    num_classes=classes, topk_sa=6, max_num_embedding=20, two_stage_num_proposals=proposals)
    tr.static_proposals = True
    crit = HybridSetCriterion(classes, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), weights)
    det = SalienceDETR(_StubBackbone(), ChannelMapper([32, 64, 64], 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=classes, num_queries=proposals, denoising_nums=12, **kw)
    det.load_state_dict(syn.det_state_dict(det.state_dict(), salt=9))
    return det.cuda().train()


def test_training_mode_ignores_the_resize():
    from salience_detr_amd import denoising as D
    g = torch.Generator().manual_seed(11)
    sizes, counts = [(64, 96), (48, 80)], (3, 2)
    images = [torch.randn(3, h, w, generator=g).cuda() for h, w in sizes]
    targets = []
    for n, (h, w) in zip(counts, sizes):
        x0, y0 = torch.rand(n, generator=g) * 0.5 * w, torch.rand(n, generator=g) * 0.5 * h
        bw, bh = torch.rand(n, generator=g) * 0.4 * w + 4, torch.rand(n, generator=g) * 0.4 * h + 4
        targets.append({"boxes": torch.stack((x0, y0, x0 + bw, y0 + bh), -1), "labels": torch.randint(0, 7, (n,), generator=g)})
    plain, sized = _train_detector(), _train_detector(min_size=128, max_size=160)
    gen = plain.denoising_generator
    shape = gen.noise_shape(len(counts), max(counts), D.denoising_groups(gen.denoising_nums, max(counts)))
    noise = torch.rand(shape, generator=torch.Generator().manual_seed(21)).cuda()
    a, b = plain(images, targets, noise=noise), sized(images, targets, noise=noise)
    assert set(a) == set(b) and len(a) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 8: refusals -------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    img = EC.image("stretch", "f32")
    dev = img.cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EvalResize(MN, MX)(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch_images([img], resize=(MN, MX))
    with pytest.raises(ValueError, match="no fallback"):
        EvalResize(MN, MX, interpolation=InterpolationMode.NEAREST)
    with pytest.raises(ValueError, match="no fallback"):
        EvalResize(MN, MX, antialias=False)
    with pytest.raises(ValueError, match="normalize=False"):
        batch_images([dev], normalize=False, resize=(MN, MX))
    with pytest.raises(RuntimeError, match="one dtype"):
        batch_images([dev, EC.image("stretch", "u8").cuda()], resize=(MN, MX))
    with pytest.raises(RuntimeError, match="float32 or uint8"):
        EvalResize(MN, MX)(dev.half())
    with pytest.raises(RuntimeError, match=r"\[3, h, w\]"):
        EvalResize(MN, MX)(dev[:1])
    with pytest.raises(ValueError, match="at most 64"):
        batch_images([dev] * 65, resize=(MN, MX))
    with pytest.raises(ValueError, match="at most 64"):
        resize_images([dev] * 65, [(8, 8)] * 65)
    with pytest.raises(ValueError, match="without pixels"):
        batch_images([torch.zeros(3, 1, 300, device="cuda")], resize=(MN, MX))
    torch.cuda.synchronize()
    canvas, _ = batch_images([dev] * 64, resize=(MN, MX))                 # 64 is served
    assert tuple(canvas.shape) == (64, 3, 64, 96) and torch.equal(canvas[0], canvas[63])
