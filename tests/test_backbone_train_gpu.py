"""GPU: training the ResNet backbone in HIP (``ResNetBackbone.set_train_form("hip")``, csrc/backbone_backward.hip).

Per-op contracts hold ``sdetr_backbone_dgrad`` / ``sdetr_backbone_wgrad`` to the float64 ``F.conv2d`` autograd on the
folded weight.  The whole-net tests deal with the ReLU problem by making the masks an input of the comparison
(tests/backbone_train_cases.py): G2 requires the HIP forward's masks to agree with the reference's float64 masks up to a
handful of elements, G3 compares the HIP gradients with the float64 masked restatement under the HIP run's OWN masks
(tied to the imported reference by G1, tests/test_backbone_train_cpu.py) against the reference's own fp32 / bf16-autocast
error under fixed masks (``d32`` / ``dbf16`` of tests/golden/backbone_train.npz).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backbone_cases as BC
import backbone_train_cases as TC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.backbone import FrozenBatchNorm2d, ResNetBackbone

pytestmark = pytest.mark.gpu
GRAD_FLOOR = 5e-6   # as tests/test_detector_train_gpu.py


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


# ---- kernels against their ABI contract ----------------------------------------------------------------------------

def _bn(co, seed):
    g = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(co)
    bn.weight.copy_(1 + 0.1 * torch.randn(co, generator=g))
    bn.bias.copy_(0.05 * torch.randn(co, generator=g))
    bn.running_mean.copy_(0.1 * torch.randn(co, generator=g))
    bn.running_var.copy_(0.5 + torch.rand(co, generator=g))
    return bn


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).cuda()


OP_CASES = [(1, 1, 64, 32), (1, 2, 64, 128), (3, 1, 32, 64), (3, 2, 64, 72), (3, 1, 96, 8)]   # (k, stride, in, out)
_op_cache = {}


def _op_case(case, precision):
    """Operands and the float64 / CPU-fp32 autograd references of one case, computed once."""
    if (case, precision) in _op_cache:
        return _op_cache[case, precision]
    k, s, ci, co = case
    g = torch.Generator().manual_seed(k * 1000 + s * 100 + ci + co)
    B, H, W = 2, 29, 37
    p = (k - 1) // 2
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    dz = torch.randn(B, co, ho, wo, generator=g)
    add = torch.randn(B, ci, H, W, generator=g)
    mask = torch.randn(B, ci, H, W, generator=g)        # random signs: no element near a flip
    bn = _bn(co, 7 + k)
    if precision == 1:   # the 16-bit operands the kernels see
        x, dz, add, mask = (t.bfloat16().float() for t in (x, dz, add, mask))
    scale = (bn.weight.double() / (bn.running_var.double() + bn.eps).sqrt())

    def grads(dt):
        xx = x.to(dt).requires_grad_(True)
        ww = w.to(dt).requires_grad_(True)
        y = F.conv2d(xx, ww * scale.to(dt).view(-1, 1, 1, 1), None, stride=s, padding=p)
        dx, dw = torch.autograd.grad(y, (xx, ww), dz.to(dt))
        return dx.double(), dw.double()
    dx64, dw64 = grads(torch.float64)
    dx32, dw32 = grads(torch.float32)
    _op_cache[case, precision] = dict(x=x, w=w, dz=dz, add=add, mask=mask, bn=bn, dx64=dx64, dw64=dw64,
                                      d32_dx=(dx32 - dx64).abs().max().item(), d32_dw=(dw32 - dw64).abs().max().item(),
                                      dims=(B, H, W, p, ho, wo))
    return _op_cache[case, precision]


def _pack_dgrad(w, bn, precision, lib):
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    f32 = [t.float().contiguous().cuda() for t in (w, bn.weight, bn.running_var)]
    packed = torch.empty(lib.sdetr_backbone_dgrad_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16, device="cuda")
    scale = torch.empty(co, device="cuda")
    _hip.check(lib.sdetr_backbone_pack_dgrad(_hip.stream_ptr(), *[t.data_ptr() for t in f32], bn.eps, co, ci, k, precision,
                                             packed.data_ptr(), scale.data_ptr()), "pack dgrad", lib)
    return packed, scale


def _bound(precision, d32, scale):
    return max(3 * d32, 2e-6 * scale) if precision == 0 else 2e-2 * scale


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("case", OP_CASES)
def test_dgrad_contract(case, with_add, with_mask, splits, precision):
    k, s, ci, co = case
    c = _op_case(case, precision)
    B, H, W, p, ho, wo = c["dims"]
    lib = _hip.lib()
    act = torch.float32 if precision == 0 else torch.bfloat16
    packed, _ = _pack_dgrad(c["w"], c["bn"], precision, lib)
    dz, add, mask = _nhwc(c["dz"], act), _nhwc(c["add"], act), _nhwc(c["mask"], act)
    out = torch.full((B, H, W, ci), float("nan"), dtype=act, device="cuda")   # every element must be written
    op = (_hip.BackboneBwdOpStruct * 1)(_hip.BackboneBwdOpStruct(
        0, dz.data_ptr(), None, packed.data_ptr(), None, add.data_ptr() if with_add else None,
        mask.data_ptr() if with_mask else None, out.data_ptr(), B, ci, H, W, co, k, s, p, splits))
    resolved = lib.sdetr_backbone_bwd_splits(op, precision)
    assert resolved >= 1 and (splits == 0 or resolved <= splits)
    nbytes = lib.sdetr_backbone_bwd_workspace_bytes(op, 1, precision)
    assert (nbytes > 0) == (resolved > 1)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_backbone_dgrad(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "dgrad", lib)
    torch.cuda.synchronize()
    got = out.cpu().double().permute(0, 3, 1, 2)
    ref = c["dx64"]
    if k == 1 and s == 2 and not with_add:   # the stride-2 1x1 gradient is exactly zero off the even pixels
        off = torch.ones(H, W, dtype=torch.bool)
        off[::2, ::2] = False
        assert (got[:, :, off] == 0).all()
    if with_add:
        ref = ref + c["add"].double()
    if with_mask:
        ref = ref * (c["mask"] > 0)
    scale = ref.abs().max().item()
    d = (got - ref).abs().max().item()
    assert d <= _bound(precision, c["d32_dx"], scale), (d, c["d32_dx"], scale)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("case", OP_CASES)
def test_wgrad_contract(case, splits, precision):
    k, s, ci, co = case
    c = _op_case(case, precision)
    B, H, W, p, ho, wo = c["dims"]
    lib = _hip.lib()
    act = torch.float32 if precision == 0 else torch.bfloat16
    _, scale_t = _pack_dgrad(c["w"], c["bn"], precision, lib)
    dz, x = _nhwc(c["dz"], act), _nhwc(c["x"], act)
    out = torch.full((co, ci, k, k), float("nan"), device="cuda")
    op = (_hip.BackboneBwdOpStruct * 1)(_hip.BackboneBwdOpStruct(
        1, dz.data_ptr(), x.data_ptr(), None, scale_t.data_ptr(), None, None, out.data_ptr(), B, ci, H, W, co, k, s, p, splits))
    resolved = lib.sdetr_backbone_bwd_splits(op, precision)
    assert resolved == 3 if splits == 3 else resolved >= 1
    nbytes = lib.sdetr_backbone_bwd_workspace_bytes(op, 1, precision)
    assert nbytes == (resolved * co * ci * k * k * 4 if resolved > 1 else 0)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_backbone_wgrad(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "wgrad", lib)
    again = torch.empty_like(out)
    op[0].out = again.data_ptr()
    _hip.check(lib.sdetr_backbone_wgrad(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "wgrad", lib)
    torch.cuda.synchronize()
    assert torch.equal(out, again)   # no atomics
    ref = c["dw64"]
    d = (out.cpu().double() - ref).abs().max().item()
    assert d <= _bound(precision, c["d32_dw"], ref.abs().max().item()), (d, c["d32_dw"], ref.abs().max().item())


def test_bad_ops_are_rejected_before_any_launch():
    lib = _hip.lib()
    mk = lambda kind, ci=64, co=32, k=3, s=1, p=1: (_hip.BackboneBwdOpStruct * 1)(_hip.BackboneBwdOpStruct(
        kind, 16, 16, 16, 16, None, None, 16, 1, ci, 8, 8, co, k, s, p, 0))
    assert lib.sdetr_backbone_dgrad(None, mk(0, ci=48), 0, None, 0) == _hip.EINVAL and b"in_channels" in lib.sdetr_last_error()
    assert lib.sdetr_backbone_wgrad(None, mk(1, k=5, p=2), 0, None, 0) == _hip.EINVAL and b"unsupported" in lib.sdetr_last_error()
    assert lib.sdetr_backbone_dgrad(None, mk(1), 0, None, 0) == _hip.EINVAL
    assert lib.sdetr_backbone_bwd_run(None, mk(7), 1, 0, None, 0) == _hip.EINVAL and b"kind" in lib.sdetr_last_error()
    assert lib.sdetr_backbone_bwd_workspace_bytes(mk(0, s=3), 1, 0) == -1


# ---- the whole backbone ---------------------------------------------------------------------------------------------

def _model(case, dtype=torch.float32, form="hip", salt=None):
    arch, ret, _ = BC.CASES[case]
    m = ResNetBackbone(arch, return_indices=ret, freeze_indices=TC.FREEZE)
    m.load_state_dict(BC.state(m.state_dict(), case) if salt is None else BC.syn.det_state_dict(m.state_dict(), salt=salt))
    return m.eval().cuda().set_dtype(dtype).set_train_form(form)


def _canvas(case):
    return BC.canvas_and_mask(BC.images(case))[0].cuda()


def _step(m, x, case, cots=None):
    """One forward + backward with the case's cotangents; returns (outputs, cotangents)."""
    outs = m(x)
    if cots is None:
        cots = {k: v.cuda() for k, v in TC.cotangents(case, outs).items()}
    torch.autograd.backward([outs[k] for k in outs], [cots[k] for k in outs])
    return outs, cots


def _grads(m):
    return {n + ".weight": c.weight.grad for n, c in m._trainable_convs()}


_runs = {}


def _hip_run(case, dtype):
    """The "hip" form's masks and gradients of one case, computed once: (masks NCHW bool on the CPU, {name: grad})."""
    if (case, dtype) not in _runs:
        m, x = _model(case, dtype), _canvas(case)
        outs, _ = _step(m, x, case)
        masks = [(t > 0).permute(0, 3, 1, 2).cpu() for _, t in m.saved_activations()]
        torch.cuda.synchronize()
        for n, p in m.named_parameters():
            assert (p.grad is None) == (not p.requires_grad), n
        _runs[case, dtype] = (masks, {n: g.detach().cpu().double() for n, g in _grads(m).items()},
                              {n: (g.dtype, g.shape, g.is_contiguous()) for n, g in _grads(m).items()})
    return _runs[case, dtype]


_oracles = {}


def _oracle(case, dtype):
    """float64 masked restatement on the CPU under the HIP run's own masks."""
    if (case, dtype) not in _oracles:
        masks, grads, _ = _hip_run(case, dtype)
        arch, ret, _ = BC.CASES[case]
        m = ResNetBackbone(arch, return_indices=ret, freeze_indices=TC.FREEZE)
        m.load_state_dict(BC.state(m.state_dict(), case))
        m = m.eval().double()
        canvas, _ = BC.canvas_and_mask(BC.images(case))
        _oracles[case, dtype] = TC.masked_grads(m, canvas, m.num_stages, m.return_indices, list(grads), case, masks=masks)
    return _oracles[case, dtype]


@pytest.mark.parametrize("case", TC.CASES)
def test_g2_forward_masks_agree_with_the_reference(gold, case):
    """A condition, not a measurement: keeps a wrong stored activation from passing G3 against itself.  The reference's
    own fp32 run differs from its float64 run in 1 (r18) / 0 (r50) elements."""
    masks, _, _ = _hip_run(case, torch.float32)
    ref = TC.unpack_masks(gold[f"{case}.masks"], gold[f"{case}.mask_shapes"])
    assert [tuple(m.shape) for m in masks] == [tuple(m.shape) for m in ref]
    flips = sum(int((a != b).sum()) for a, b in zip(masks, ref))
    print(case, "mask elements that differ from the reference's float64 run:", flips)
    assert flips <= 16


def _compare(gold, case, dtype, factor, key, floor):
    _, grads, meta = _hip_run(case, dtype)
    ref = _oracle(case, dtype)
    assert list(grads) == [str(n) for n in gold[f"{case}.names"]]
    worst_ratio, worst_floor, failures = 0.0, 0.0, []
    for n, g in grads.items():
        assert meta[n][0] == torch.float32 and meta[n][2] and torch.isfinite(g).all(), n
        idx = TC.stored_index(g.numel())
        scale = ref[n].abs().max().item()
        own = TC.own_scale(g.reshape(-1)[idx], ref[n].reshape(-1)[idx], scale)
        rel = abs(g.norm().item() - ref[n].norm().item()) / ref[n].norm().item()
        d_ref = float(gold[f"{case}.{key}:{n}"])
        bar = max(factor * d_ref, floor)
        print(f"{case} {n:34s} own-scale {own:.2e} norm {rel:.2e} d_ref {d_ref:.2e} bar {bar:.2e}")
        for v in (own, rel):
            if factor * d_ref >= floor:
                worst_ratio = max(worst_ratio, v / d_ref)
            else:
                worst_floor = max(worst_floor, v)
            if not v <= bar:
                failures.append((n, v, bar))
    print(f"{case} {dtype}: worst ratio to d_ref {worst_ratio:.2f}, worst floor-decided value {worst_floor:.2e}")
    assert not failures, failures


@pytest.mark.parametrize("case", TC.CASES)
def test_g3_fp32_gradients_within_the_reference_error(gold, case):
    """Every stored element and every norm within ``max(4 * d32, GRAD_FLOOR)`` of the float64 masked restatement under
    the HIP run's own masks, on the tensor's own scale.  ``d32`` (5e-8 .. 6e-7) times 4 lies below the floor for every
    tensor, so the floor decides.  The test prints each figure, the worst ratio and the worst floor-decided value; none
    has been recorded here yet (no MI355X run of this file has been made)."""
    _compare(gold, case, torch.float32, 4, "d32", GRAD_FLOOR)


@pytest.mark.parametrize("case", TC.CASES)
def test_g3_bf16_gradients_within_the_reference_autocast_error(gold, case):
    """bf16 mode: within ``2 * dbf16`` (the reference under ``torch.autocast("cpu", bfloat16)`` with fixed masks) of the
    float64 masked restatement under the HIP run's own masks.  The worst ratio is printed; none has been recorded here
    yet (no MI355X run of this file has been made)."""
    _compare(gold, case, torch.bfloat16, 2, "dbf16", 0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical_accumulation_and_graph_replay(dtype):
    case = "r18"
    m, x = _model(case, dtype), _canvas(case)
    # (no step's outputs are kept: a live autograd graph keeps its AccumulateGrad nodes, which carry the stream they were
    # made on -- here the default stream -- and every later forward reuses them; the captured backward would then pull the
    # default stream into the capture, which a hipGraph capture does not survive)
    cots = _step(m, x, case)[1]
    first = {n: g.clone() for n, g in _grads(m).items()}
    _step(m, x, case, cots)                       # a second backward() accumulates
    torch.cuda.synchronize()
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n] + first[n]), n
    m.zero_grad(set_to_none=True)
    _step(m, x, case, cots)
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n]), n        # two runs, bit for bit
    # forward + backward as one captured graph, gradients accumulated into the existing .grad buffers
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _step(m, x, case, cots)                   # eager warm-up on the side stream
        torch.cuda.synchronize()
        for g in _grads(m).values():
            g.zero_()
        with torch.cuda.graph(graph, stream=stream):
            _step(m, x, case, cots)
    torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    for g in _grads(m).values():
        g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n]), n


def test_new_state_dict_repacks_the_backward_weights():
    case = "r18"
    m, x = _model(case), _canvas(case)
    cots = _step(m, x, case)[1]
    m.load_state_dict(BC.syn.det_state_dict(m.state_dict(), salt=77))
    m.zero_grad(set_to_none=True)
    _step(m, x, case, cots)
    fresh = _model(case, salt=77)
    _step(fresh, x, case, cots)
    torch.cuda.synchronize()
    a, b = _grads(m), _grads(fresh)
    for n in a:
        assert torch.equal(a[n], b[n]), n


def test_hip_request_that_is_not_eligible_raises_at_forward():
    arch, ret, _ = BC.CASES["r18"]
    m = ResNetBackbone(arch, return_indices=ret).cuda().set_train_form("hip")   # stem not frozen
    with pytest.raises(RuntimeError, match="stem"):
        m(_canvas("r18"))
    m = _model("r18", torch.float16)
    with pytest.raises(RuntimeError, match="float16"):
        m(_canvas("r18"))


# ---- the detector ---------------------------------------------------------------------------------------------------

def test_detector_trains_its_backbone_in_hip():
    import test_detector_train_gpu as T
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.optimizer import ClippedAdamW
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.salience_transformer import build_salience_transformer
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion

    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2,
                                    num_decoder_layers=T.DEC_LAYERS, num_classes=T.C, topk_sa=6, max_num_embedding=20,
                                    two_stage_num_proposals=T.PROPOSALS)
    tr.static_proposals = True
    crit = HybridSetCriterion(T.C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), T.weight_dict())
    backbone = ResNetBackbone("resnet18", return_indices=(1, 2, 3), freeze_indices=(0,))
    det = SalienceDETR(backbone, ChannelMapper([128, 256, 512], 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=T.C, num_queries=T.PROPOSALS, denoising_nums=12)
    det.load_state_dict(BC.syn.det_state_dict(det.state_dict(), salt=9))
    det = det.cuda().train()
    images, targets = T.batch()
    noise = T.noise_for(det, (3, 2))
    losses = {}
    for form in ("torch", "hip"):
        backbone.set_train_form(form)
        det.zero_grad(set_to_none=True)
        losses[form] = det(images, targets, noise=noise)
    assert list(losses["hip"]) == list(losses["torch"])
    for k, v in losses["torch"].items():
        assert abs(losses["hip"][k].item() - v.item()) <= 2e-3 * max(1.0, abs(v.item())), k
    sum(losses["hip"].values()).backward()
    convs = backbone._trainable_convs()
    assert len(convs) == 15
    for n, c in convs:
        g = c.weight.grad
        assert g is not None and g.dtype == torch.float32 and g.shape == c.weight.shape and g.is_contiguous(), n
        assert torch.isfinite(g).all() and g.abs().max().item() > 0, n
    assert backbone.conv1.weight.grad is None and all(p.grad is None for p in backbone.layer1.parameters())
    ClippedAdamW([p for p in det.parameters() if p.requires_grad], lr=1e-4).step()
    torch.cuda.synchronize()
