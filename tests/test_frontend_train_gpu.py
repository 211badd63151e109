"""GPU: training the ChannelMapper in HIP (``ChannelMapper.set_train_form("hip")``, csrc/frontend_backward.hip).

The GroupNorm backward kind is held to float64 torch autograd, on the CPU, of ``F.group_norm`` on the kernel's own ``z``
(the raw convolution the training forward stored), the egest kind to ``permute`` + add, exactly.  fp32 bar: ``max(3 * d32,
2e-6 * scale)`` with ``d32`` the distance of the CPU fp32 autograd run from float64; 16-bit bar of ``dz``: ``max(2e-2 *
scale, 1.5 * dbf)`` with ``dbf`` the distance of the CPU autograd under ``torch.autocast(bfloat16)`` from float64, as
tests/test_swin_train_gpu.py; ``dgamma`` / ``dbeta`` are fp32 sums of fp32 terms in both precisions (the reference sees the
same rounded ``add``) and are held to the fp32 bar.  ``scale`` is the reference tensor's max abs; of the stored mean it is
max|z| (an fp32 mean of values of that size errs by a multiple of their ulp, whatever the mean itself is), of rstd its own
max.  The whole-mapper tests compare every parameter and input gradient with the imported reference's float64 gradients
(tests/golden/frontend_train.npz) against the reference's own fp32 / bf16-autocast error.  Every test prints its worst
value / bar; first MI355X run: GroupNorm backward fp32 0.09 (dz) / 0.30 (dgamma) / 0.05 (dbeta), bf16 0.15 / 0.17 / 0.05;
statistics 0.02 (mean) / 0.05 (rstd); the 3x3 level's z 0.22; whole mapper fp32 0.07 / 0.08 / 0.06 / 0.10 and bf16 0.22 /
0.23 / 0.20 / 0.73 (t4 / x2 / g16 / r50)."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import frontend_train_cases as TC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.channel_mapper import ChannelMapper

pytestmark = pytest.mark.gpu
GRAD_FLOOR = 5e-6   # as tests/test_backbone_train_gpu.py
B = 2


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


def _act(precision):
    return torch.float32 if precision == 0 else torch.bfloat16


def _op(**fields):
    return _hip.FrontendBwdOpStruct(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in fields.items()})


def _run(precision, **fields):
    """One ``sdetr_frontend_bwd_op_run``; tensors in ``fields`` become their pointers."""
    lib = _hip.lib()
    op = (_hip.FrontendBwdOpStruct * 1)(_op(**fields))
    nbytes = lib.sdetr_frontend_bwd_workspace_bytes(op, 1, precision)
    _hip.check(0 if nbytes >= 0 else -1, "frontend bwd workspace", lib)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_frontend_bwd_op_run(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "frontend bwd op", lib)
    torch.cuda.synchronize()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")   # every element must be written


def _bar(r64, r32, rbf, precision, scale=None):
    scale = r64.abs().max().item() if scale is None else scale
    if precision == 0:
        return max(3 * (r32.double() - r64).abs().max().item(), 2e-6 * scale)
    return max(2e-2 * scale, 1.5 * (rbf.double() - r64).abs().max().item())


def _check(what, got, r64, r32, rbf, precision, worst, scale=None):
    err = (got.detach().cpu().double() - r64).abs().max().item()
    bar = _bar(r64, r32, rbf, precision, scale)
    worst[what] = max(worst.get(what, 0.0), err / bar)
    assert torch.isfinite(got).all() and err <= bar, (what, err, bar)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _group_norm_grads(z, cot, gamma, groups, eps, dtype, autocast=None):
    zz, g = z.to(dtype).requires_grad_(True), gamma.to(dtype).requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            y = F.group_norm(zz, groups, g, b, eps)
    else:
        y = F.group_norm(zz, groups, g, b, eps)
    return [t.double() for t in torch.autograd.grad((y.double() * cot.double()).sum(), (zz, g, b))]


def _statistics(z, groups, eps, dtype):
    v = z.to(dtype).reshape(z.shape[0], groups, -1)
    mean = v.mean(-1)
    return mean.double(), (1.0 / torch.sqrt(((v - mean[..., None]) ** 2).mean(-1) + eps)).double()


GROUP_NORM = [(64, 32, 3, 4), (48, 16, 13, 20), (256, 32, 1, 2), (64, 32, 1, 1), (256, 32, 11, 16)]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", GROUP_NORM)
def test_group_norm_backward_kind(shape, precision):
    co, groups, h, w = shape
    act, worst, eps = _act(precision), {}, 1e-5
    # z and the statistics are the training forward's own: a one-level mapper over a random map
    m = ChannelMapper([32], co, 1, norm_layer=partial(nn.GroupNorm, groups, eps=eps))
    gamma = 1 + 0.2 * _rand(1, co)
    gamma[list(TC.ZERO_GAMMA)] = 0.0
    m.load_state_dict({"convs.0.0.weight": 0.3 * _rand(2, co, 32, 1, 1), "convs.0.1.weight": gamma, "convs.0.1.bias": _rand(3, co)})
    m = m.cuda().set_dtype(act)
    state = {}
    with torch.no_grad():
        m.forward_hip([_rand(4, B, 32, h, w).cuda()], state)
    z, stats = state["acts"]["convs.0.z"], state["acts"]["convs.0.stats"]
    zc = z.cpu()
    mean64, rstd64 = _statistics(zc, groups, eps, torch.float64)
    mean32, rstd32 = _statistics(zc, groups, eps, torch.float32)
    _check("mean", stats[..., 0], mean64, mean32, None, 0, worst, scale=zc.abs().max().item())
    _check("rstd", stats[..., 1], rstd64, rstd32, None, 0, worst)
    dy = _rand(5, B, co, h, w)
    add = _rand(6, B, h, w, co).to(act)            # the reference sees the same rounded add
    for with_add in (True, False):
        cot = dy + add.float().permute(0, 3, 1, 2) if with_add else dy
        r64 = _group_norm_grads(zc, cot, gamma, groups, eps, torch.float64)
        r32 = _group_norm_grads(zc, cot, gamma, groups, eps, torch.float32)
        rbf = _group_norm_grads(zc, cot, gamma, groups, eps, torch.float32, torch.bfloat16) if precision else r32
        dz, dg, db = _nan((B, h, w, co), act), _nan((co,)), _nan((co,))
        _run(precision, kind=3, dz=dy.cuda(), add=add.cuda() if with_add else None, z=z, stats=stats, gamma=gamma.cuda(), out=dz,
             dgamma=dg, dbeta=db, batch=B, height=h, width=w, out_channels=co, groups=groups, eps=eps)
        _check("dz", dz.float().permute(0, 3, 1, 2), r64[0], r32[0], rbf[0], precision, worst)
        _check("dgamma", dg, r64[1], r32[1], rbf[1], 0, worst)
        _check("dbeta", db, r64[2], r32[2], rbf[2], 0, worst)
        assert r64[1][list(TC.ZERO_GAMMA)].abs().min().item() > 0      # a zero gamma still has a gradient
        only = _nan((B, h, w, co), act)                                  # dgamma and dbeta are optional, together
        _run(precision, kind=3, dz=dy.cuda(), add=add.cuda() if with_add else None, z=z, stats=stats, gamma=gamma.cuda(), out=only,
             batch=B, height=h, width=w, out_channels=co, groups=groups, eps=eps)
        assert torch.equal(only, dz)
    print(shape, precision, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", [(64, 3, 4), (96, 5, 7), (2048, 2, 3)])
def test_egest_kind_is_exact(shape, precision):
    c, h, w = shape
    act = _act(precision)
    a, b = _rand(7, B, h, w, c).to(act).cuda(), _rand(8, B, h, w, c).to(act).cuda()
    for second in (b, None):
        out = _nan((B, c, h, w))
        _run(precision, kind=4, dz=a, add=second, out=out, batch=B, in_channels=c, height=h, width=w)
        ref = a.float() if second is None else a.float() + second.float()
        assert torch.equal(out, ref.permute(0, 3, 1, 2))


def test_a_bad_backward_op_is_rejected_before_any_launch():
    lib = _hip.lib()
    co, groups, h, w = 64, 32, 3, 4
    t = torch.zeros(B * h * w * co + 4096, device="cuda")
    good = dict(kind=3, dz=t, z=t, stats=t, gamma=t, out=t[4096:], dgamma=t[64:], dbeta=t[128:], batch=B, height=h, width=w,
                out_channels=co, groups=groups, eps=1e-5)
    for bad, text in ((dict(z=None), "null"), (dict(groups=7), "groups"), (dict(gamma=t[1:]), "aligned"), (dict(), "workspace")):
        first = dict(kind=4, dz=t, out=_nan((B, co, h, w)), batch=B, in_channels=co, height=h, width=w)
        ops = (_hip.FrontendBwdOpStruct * 2)(_op(**first), _op(**{**good, **bad}))
        need = lib.sdetr_frontend_bwd_workspace_bytes(ops, 2, 0)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        if bad:
            assert need == -1
            rc = lib.sdetr_frontend_bwd_run(_hip.stream_ptr(), ops, 2, 0, ws.data_ptr(), ws.numel())
        else:            # a valid plan over a workspace that is too small
            assert 16 < need <= ws.numel()
            rc = lib.sdetr_frontend_bwd_run(_hip.stream_ptr(), ops, 2, 0, ws.data_ptr(), need - 16)
        assert rc == _hip.EINVAL
        assert text in lib.sdetr_last_error().decode(), (bad, lib.sdetr_last_error())
        torch.cuda.synchronize()
        assert torch.isnan(first["out"]).all()           # the valid first op did not run


# ---- the whole mapper -----------------------------------------------------------------------------------------------

def _model(case, dtype=torch.float32, form="hip", salt=None):
    m = TC.build(ChannelMapper, case)
    if salt is not None:
        m.load_state_dict(TC.state(m.state_dict(), case, salt=salt))
    return m.cuda().train().set_dtype(dtype).set_train_form(form)


def _inputs(case, grad=True):
    return [x.cuda().requires_grad_(grad) for x in TC.inputs(case)]


def _step(m, xs, case, cots=None):
    outs = m(xs)
    if cots is None:
        cots = [c.cuda() for c in TC.cotangents(case, outs)]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    return cots


def _grads(m, xs=()):
    got = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    got.update({f"input.{l}": x.grad for l, x in enumerate(xs)})
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(TC.CASES))
def test_training_forward_equals_the_inference_forward_and_stores_the_convolution(case, dtype):
    m, xs = _model(case, dtype), _inputs(case)
    outs = m(xs)
    acts = m.saved_activations()
    with torch.no_grad():
        ref = m.forward_hip(xs)
    assert len(outs) == len(ref) == len(m.convs)
    for a, b in zip(outs, ref):
        assert a.dtype == torch.float32 and a.requires_grad and torch.equal(a, b)
    nin = len(xs)
    assert all(acts[f"input.{l}"].data_ptr() == x.data_ptr() for l, x in enumerate(xs))   # the inputs are not copied
    if dtype == torch.float32:   # the 3x3 level's z, the sum of the split-K partials, is the convolution
        w = m.convs[nin][0].weight.detach().cpu()
        r64 = F.conv2d(xs[-1].detach().cpu().double(), w.double(), stride=2, padding=1)
        r32 = F.conv2d(xs[-1].detach().cpu(), w, stride=2, padding=1)
        worst = {}
        _check("z", acts[f"convs.{nin}.z"], r64, r32, None, 0, worst)
        print(case, worst)


def _compare(gold, case, dtype, key):
    m, xs = _model(case, dtype), _inputs(case)
    _step(m, xs, case)
    torch.cuda.synchronize()
    names = [str(n) for n in gold[f"{case}.names"]]
    grads = _grads(m, xs)
    assert list(grads) == names
    worst, failures = 0.0, []
    for n in names:
        g = grads[n]
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), n
        g = g.cpu().double()
        idx = TC.stored_index(g.numel())
        ref, scale = torch.from_numpy(gold[f"{case}.g:{n}"]), float(gold[f"{case}.max:{n}"])
        own = TC.own_scale(g.reshape(-1)[idx], ref, scale)
        rel = abs(g.norm().item() - float(gold[f"{case}.norm:{n}"])) / float(gold[f"{case}.norm:{n}"])
        d_ref = float(gold[f"{case}.{key}:{n}"])
        bar = max(4 * d_ref, GRAD_FLOOR)
        print(f"{case} {n:24s} own-scale {own:.2e} norm {rel:.2e} d_ref {d_ref:.2e} bar {bar:.2e}")
        worst = max(worst, own / bar, rel / bar)
        failures.extend((n, v, bar) for v in (own, rel) if not v <= bar)
    print(f"{case} {dtype}: worst value / bar {worst:.2f}")
    assert not failures, failures


@pytest.mark.parametrize("case", list(TC.CASES))
def test_fp32_gradients_within_the_reference_error(gold, case):
    """Every stored element and every norm within ``max(4 * d32, GRAD_FLOOR)`` of the reference's float64 gradients, on
    the tensor's own scale."""
    _compare(gold, case, torch.float32, "d32")


@pytest.mark.parametrize("case", list(TC.CASES))
def test_bf16_gradients_within_the_reference_autocast_error(gold, case):
    """bf16 mode: bounded the same way by the reference's ``torch.autocast("cpu", bfloat16)`` distance ``dbf16``."""
    _compare(gold, case, torch.bfloat16, "dbf16")


@pytest.mark.parametrize("case", ["t4", "x2"])
def test_inputs_without_grad_get_none_and_the_parameter_gradients_do_not_change(case):
    m, xs = _model(case), _inputs(case)
    cots = _step(m, xs, case)
    full = {n: g.clone() for n, g in _grads(m).items()}
    m.zero_grad(set_to_none=True)
    frozen = _inputs(case, grad=False)
    _step(m, frozen, case, cots)
    torch.cuda.synchronize()
    assert all(x.grad is None for x in frozen)
    for n, g in _grads(m).items():
        assert torch.equal(g, full[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical_accumulation_and_graph_replay(dtype):
    case = "x2"
    m, xs = _model(case, dtype), _inputs(case)
    cots = _step(m, xs, case)
    first = {n: g.clone() for n, g in _grads(m, xs).items()}
    _step(m, xs, case, cots)                      # a second backward() accumulates
    torch.cuda.synchronize()
    for n, g in _grads(m, xs).items():
        assert torch.equal(g, first[n] + first[n]), n

    def clear():
        m.zero_grad(set_to_none=True)
        for x in xs:
            x.grad = None
    clear()
    _step(m, xs, case, cots)
    for n, g in _grads(m, xs).items():
        assert torch.equal(g, first[n]), n        # two runs, bit for bit
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _step(m, xs, case, cots)                  # eager warm-up on the side stream
        torch.cuda.synchronize()
        for g in _grads(m, xs).values():
            g.zero_()
        with torch.cuda.graph(graph, stream=stream):
            _step(m, xs, case, cots)
    torch.cuda.current_stream().wait_stream(stream)
    for replay in range(2):
        for g in _grads(m, xs).values():
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n, g in _grads(m, xs).items():
            assert torch.equal(g, first[n]), (replay, n)


def test_new_state_dict_repacks_the_backward_data_planes():
    case = "x2"
    m, xs = _model(case), _inputs(case)
    cots = _step(m, xs, case)
    before = {n: g.clone() for n, g in _grads(m, xs).items()}
    m.load_state_dict(TC.state(m.state_dict(), case, salt=77))
    m.zero_grad(set_to_none=True)
    for x in xs:
        x.grad = None
    _step(m, xs, case, cots)
    fresh, ys = _model(case, salt=77), _inputs(case)
    _step(fresh, ys, case, cots)
    torch.cuda.synchronize()
    a, b = _grads(m, xs), _grads(fresh, ys)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert all(not torch.equal(a[f"input.{l}"], before[f"input.{l}"]) for l in range(len(xs)))   # through the dgrad planes


def test_hip_request_that_is_not_eligible_raises_at_forward():
    case = "x2"
    with pytest.raises(RuntimeError, match="float16"):
        _model(case, torch.float16)(_inputs(case))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        _model(case)([x.requires_grad_(True) for x in TC.inputs(case)])
    narrow = ChannelMapper([64], 12, 1, norm_layer=partial(nn.GroupNorm, 4)).cuda().set_train_form("hip")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        narrow([torch.zeros(1, 64, 4, 4, device="cuda")])
    other = ChannelMapper([48], 64, 1).cuda().set_train_form("hip")
    with pytest.raises(RuntimeError, match="not one the HIP kernels serve"):
        other([torch.zeros(1, 48, 4, 4, device="cuda")])


def test_detector_trains_its_neck_in_hip():
    import swin_cases as SC
    import test_detector_train_gpu as T
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.salience_transformer import build_salience_transformer
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion
    from salience_detr_amd.swin import SwinBackbone

    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2,
                                    num_decoder_layers=T.DEC_LAYERS, num_classes=T.C, topk_sa=6, max_num_embedding=20,
                                    two_stage_num_proposals=T.PROPOSALS)
    tr.static_proposals = True
    crit = HybridSetCriterion(T.C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), T.weight_dict())
    backbone = SwinBackbone(None, return_indices=(1, 2, 3), freeze_indices=(0,), embed_dim=32, depths=(1, 2, 2, 1),
                            num_heads=(1, 2, 4, 8), window_size=(7, 7), stochastic_depth_prob=0.0)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=T.C, num_queries=T.PROPOSALS, denoising_nums=12)
    sd = SC.syn.det_state_dict(det.state_dict(), salt=9)
    sd.update({"backbone." + k: v for k, v in SC.state(backbone.state_dict(), "det").items()})
    det.load_state_dict(sd)
    det = det.cuda().train()
    backbone.set_train_form("hip")
    images, targets = T.batch()
    noise = T.noise_for(det, (3, 2))
    losses = {}
    for form in ("torch", "hip"):
        det.neck.set_train_form(form)
        det.zero_grad(set_to_none=True)
        losses[form] = det(images, targets, noise=noise)
    assert list(losses["hip"]) == list(losses["torch"])
    for k, v in losses["torch"].items():
        assert abs(losses["hip"][k].item() - v.item()) <= 2e-3 * max(1.0, abs(v.item())), k
    sum(losses["hip"].values()).backward()
    trainable = [("neck." + n, p) for n, p in det.neck.named_parameters() if p.requires_grad] + backbone._trainable()
    assert len(trainable) > len(backbone._trainable()) > 0
    for n, p in trainable:
        g = p.grad
        assert g is not None and g.dtype == torch.float32 and g.shape == p.shape, n
        assert torch.isfinite(g).all() and g.abs().max().item() > 0, n
    torch.cuda.synchronize()
