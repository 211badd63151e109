"""GPU: training the ConvNeXt backbone in HIP (``ConvNeXtBackbone.set_train_form("hip")``, csrc/convnext_backward.hip).

Per-kind contracts hold ``sdetr_convnext_bwd_op_run`` to float64 torch autograd of the same op on the CPU, bounded as
tests/test_backbone_train_gpu.py bounds its ops (``_bound``: three times the distance of a CPU fp32 autograd run from
float64, floored at 2e-6 of the operand scale; 2e-2 of the scale with 16-bit operands).  The whole-net tests compare the
parameter gradients with the imported reference's float64 gradients (tests/golden/convnext_train.npz) against the
reference's own fp32 / bf16-autocast error.  Every test prints its worst ratio; first MI355X run: worst value / bar 0.15
(fp32, both cases), 0.36 / 0.25 (bf16, ct1 / ct2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_cases as CC
import convnext_train_cases as TC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone

pytestmark = pytest.mark.gpu
GRAD_FLOOR = 5e-6   # as tests/test_backbone_train_gpu.py
SHAPES = [(96, 5, 7), (96, 13, 19), (1536, 5, 7), (1536, 13, 19)]   # (C, H, W): see the module docstring of the cases
B = 2


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


def _bound(precision, d32, scale):
    return max(3 * d32, 2e-6 * scale) if precision == 0 else 2e-2 * scale


def _act(precision):
    return torch.float32 if precision == 0 else torch.bfloat16


def _run(precision, **fields):
    """One ``sdetr_convnext_bwd_op_run``; tensors in ``fields`` become their pointers."""
    lib = _hip.lib()
    keep = [v for v in fields.values() if isinstance(v, torch.Tensor)]
    op = (_hip.ConvnextBwdOpStruct * 1)(_hip.ConvnextBwdOpStruct(
        **{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in fields.items()}))
    nbytes = lib.sdetr_convnext_bwd_workspace_bytes(op, 1, precision)
    _hip.check(0 if nbytes >= 0 else -1, "convnext bwd workspace", lib)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_convnext_bwd_op_run(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "convnext bwd op", lib)
    torch.cuda.synchronize()
    return keep


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")   # every element must be written


def _check(what, got, ref64, ref32, precision, worst):
    scale = ref64.abs().max().item()
    d32 = (ref32.double() - ref64).abs().max().item()
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    bar = _bound(precision, d32, scale)
    worst[what] = max(worst.get(what, 0.0), err / bar)
    assert torch.isfinite(got).all() and err <= bar, (what, err, bar, d32, scale)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_rows_and_gelu_kinds(shape, splits, precision):
    c, h, w = shape
    act, worst = _act(precision), {}
    dy = _rand(1, B, h, w, c)
    s = torch.tensor([0.0, 2.0])                         # one dropped sample, one survivor at p = 0.5
    out, db = _nan((B, h, w, c), act), _nan((c,))
    _run(precision, kind=2, dz=dy.cuda(), scale=s.cuda(), out=out, dbias=db, batch=B, channels=c, height=h, width=w, splits=splits)
    ref = dy.double() * s.double().view(B, 1, 1, 1)
    assert (out[0] == 0).all()
    _check("rows", out.float(), ref, ref.float(), precision, worst)
    _check("rows dbias", db, ref.sum((0, 1, 2)), ref.float().sum((0, 1, 2)), 0, worst)
    out2, db2 = _nan((B, h, w, c), act), _nan((c,))
    _run(precision, kind=2, dz=dy.cuda(), out=out2, dbias=db2, batch=B, channels=c, height=h, width=w, splits=splits)
    _check("rows (no scale)", out2.float(), dy.double(), dy, precision, worst)
    # GELU backward on the values the kernel sees
    dh, pre = (_rand(2, B, h, w, c).to(act).float(), (2 * _rand(3, B, h, w, c)).to(act).float())

    def grad(dt):
        p = pre.to(dt).requires_grad_(True)
        return torch.autograd.grad(F.gelu(p), p, dh.to(dt))[0]
    g64, g32 = grad(torch.float64), grad(torch.float32)
    out3, db3 = _nan((B, h, w, c), act), _nan((c,))
    _run(precision, kind=3, dz=dh.to(act).cuda(), x=pre.to(act).cuda(), out=out3, dbias=db3, batch=B, channels=c, height=h, width=w,
         splits=splits)
    _check("gelu", out3.float(), g64, g32, precision, worst)
    _check("gelu dbias", db3, g64.sum((0, 1, 2)), g32.sum((0, 1, 2)), 0, worst)
    print(shape, splits, precision, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_layer_norm_kind(shape, splits, precision):
    c, h, w = shape
    act, worst = _act(precision), {}
    x = _rand(4, B, h, w, c) * 1.5 + 0.3
    x[0, 0, 0] = 0.75                                    # a row of constant input: variance 0, eps only
    dn = _rand(5, B, h, w, c).to(act).float()
    gamma, add = 1 + 0.2 * _rand(6, c), _rand(7, B, h, w, c)

    def grads(dt):
        xx, gg, bb = x.to(dt).requires_grad_(True), gamma.to(dt).requires_grad_(True), torch.zeros(c, dtype=dt, requires_grad=True)
        y = F.layer_norm(xx, (c,), gg, bb, 1e-6)
        return torch.autograd.grad(y, (xx, gg, bb), dn.to(dt))
    r64, r32 = grads(torch.float64), grads(torch.float32)
    out, dg, db = _nan((B, h, w, c)), _nan((c,)), _nan((c,))
    _run(precision, kind=4, dz=dn.to(act).cuda(), x=x.cuda(), gamma=gamma.cuda(), add=add.cuda(), out=out, dgamma=dg, dbeta=db,
         batch=B, channels=c, height=h, width=w, splits=splits, eps=1e-6)
    _check("ln dx", out.cpu() - add, r64[0], r32[0], 0, worst)
    _check("ln dgamma", dg, r64[1], r32[1], 0, worst)
    _check("ln dbeta", db, r64[2], r32[2], 0, worst)
    print(shape, splits, precision, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_depthwise_kinds(shape, splits):
    c, h, w = shape
    worst = {}
    x, d, taps, add = _rand(8, B, c, h, w), _rand(9, B, c, h, w), _rand(10, c, 1, 7, 7) / 7, _rand(11, B, h, w, c)

    def grads(dt):
        xx, ww, bb = x.to(dt).requires_grad_(True), taps.to(dt).requires_grad_(True), torch.zeros(c, dtype=dt, requires_grad=True)
        y = F.conv2d(xx, ww, bb, padding=3, groups=c)
        return torch.autograd.grad(y, (xx, ww, bb), d.to(dt))
    r64, r32 = grads(torch.float64), grads(torch.float32)
    rows = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    dtaps, dbd = _nan((49, c)), _nan((c,))
    _run(0, kind=5, dz=rows(d), x=rows(x), out=dtaps, dbias=dbd, batch=B, channels=c, height=h, width=w, splits=splits)
    _check("dw dtaps", dtaps.t().reshape(c, 1, 7, 7), r64[1], r32[1], 0, worst)
    _check("dw dbias", dbd, r64[2], r32[2], 0, worst)
    dx = _nan((B, h, w, c))
    _run(0, kind=6, dz=rows(d), weight=taps.reshape(c, 49).t().contiguous().cuda(), add=add.cuda(), out=dx, batch=B, channels=c,
         height=h, width=w)
    _check("dw dx", (dx.cpu() - add).permute(0, 3, 1, 2), r64[0], r32[0], 0, worst)
    print(shape, splits, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("c", [96, 1536])
def test_layer_scale_and_ingest_kinds(c):
    worst, k = {}, 4 * c
    dwp, w2, b2, g, dbp = _rand(12, c, k), _rand(13, c, k), _rand(14, c), 0.1 + 0.2 * _rand(21, c).abs(), _rand(15, c)
    dw, db, dg = _nan((c, k)), _nan((c,)), _nan((c,))
    _run(0, kind=7, dz=dbp.cuda(), x=dwp.cuda(), weight=w2.cuda(), scale=b2.cuda(), gamma=g.cuda(), out=dw, dbias=db, dgamma=dg,
         batch=1, channels=c, height=1, width=1, out_channels=k)
    ref = lambda dt: (dwp.to(dt) * w2.to(dt)).sum(1) + dbp.to(dt) * b2.to(dt)
    _check("layer scale dg", dg, ref(torch.float64), ref(torch.float32), 0, worst)
    assert torch.equal(dw.cpu(), g.view(c, 1) * dwp) and torch.equal(db.cpu(), g * dbp)
    cot, add = _rand(16, B, c, 13, 19), _rand(17, B, 13, 19, c)
    out = _nan((B, 13, 19, c))
    _run(0, kind=10, dz=cot.cuda(), add=add.cuda(), out=out, batch=B, channels=c, height=13, width=19)
    assert torch.equal(out.cpu(), cot.permute(0, 2, 3, 1) + add)
    print(c, {k_: round(v, 3) for k_, v in worst.items()})


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("c", [96, 768])
def test_linear_and_down_sampler_kinds(c, splits, precision):
    """The GEMM kinds on a Linear with a folded layer scale, and the down-sampler at 13 x 19 (odd row and column) as
    patches -> wgrad / dgrad -> pixels against ``F.conv2d(k = 2, s = 2)`` autograd."""
    lib, act, worst = _hip.lib(), _act(precision), {}
    h, w, co = 13, 19, 2 * c
    ho, wo = h // 2, w // 2
    x = _rand(18, B, c, h, w).to(act).float()
    wt = _rand(19, co, c, 2, 2) / (4 * c) ** 0.5
    dz = _rand(20, B, co, ho, wo).to(act).float()

    def grads(dt):
        xx, ww = x.to(dt).requires_grad_(True), wt.to(dt).requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xx, ww, None, stride=2), (xx, ww), dz.to(dt))
    r64, r32 = grads(torch.float64), grads(torch.float32)
    rows = lambda t: t.permute(0, 2, 3, 1).contiguous().to(act).cuda()
    patches = _nan((B, ho, wo, 4 * c), act)
    _run(precision, kind=8, x=rows(x), out=patches, batch=B, channels=c, height=h, width=w)
    ones = torch.ones(co, device="cuda")
    dwp = _nan((co, 4 * c))
    _run(precision, kind=1, dz=rows(dz), x=patches, scale=ones, out=dwp, batch=B, channels=4 * c, height=ho, width=wo,
         out_channels=co, splits=splits)
    _check("down dW", dwp.view(co, 2, 2, c).permute(0, 3, 1, 2), r64[1], r32[1], precision, worst)
    w2d = wt.permute(0, 2, 3, 1).reshape(co, 4 * c).contiguous().cuda()
    packed = torch.empty(lib.sdetr_backbone_dgrad_packed_bytes(co, 4 * c, 1, precision) // 2, dtype=torch.int16, device="cuda")
    unused = torch.empty(co, device="cuda")
    _hip.check(lib.sdetr_backbone_pack_dgrad(_hip.stream_ptr(), w2d.data_ptr(), ones.data_ptr(), ones.data_ptr(), 0.0, co, 4 * c,
                                             1, precision, packed.data_ptr(), unused.data_ptr()), "pack dgrad", lib)
    dpatch = _nan((B, ho, wo, 4 * c), act)
    _run(precision, kind=0, dz=rows(dz), weight=packed, out=dpatch, batch=B, channels=4 * c, height=ho, width=wo, out_channels=co,
         splits=splits)
    dx = _nan((B, h, w, c), act)
    _run(precision, kind=9, dz=dpatch, out=dx, batch=B, channels=c, height=h, width=w)
    assert (dx[:, h - 1] == 0).all() and (dx[:, :, w - 1] == 0).all()   # the cropped row and column: exact zeros
    _check("down dx", dx.float().permute(0, 3, 1, 2), r64[0], r32[0], precision, worst)
    print(c, splits, precision, {k: round(v, 3) for k, v in worst.items()})


def test_a_bad_backward_op_is_rejected_before_any_launch():
    lib = _hip.lib()
    t = torch.zeros(2 * 5 * 7 * 96 + 8, device="cuda")
    good = dict(kind=4, dz=t, x=t, gamma=t, out=t, dgamma=t, dbeta=t, batch=2, channels=96, height=5, width=7, eps=1e-6)
    for bad, text in ((dict(channels=80), "multiple of 32"), (dict(channels=3104), "3072"), (dict(x=None), "null"),
                      (dict(out=t[1:]), "aligned"), (dict(kind=11), "unknown")):
        f = {**good, **bad}
        first = dict(kind=10, dz=t, out=_nan((2, 5, 7, 96)), batch=2, channels=96, height=5, width=7)
        ops = (_hip.ConvnextBwdOpStruct * 2)(*[_hip.ConvnextBwdOpStruct(
            **{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}) for d in (first, f)])
        assert lib.sdetr_convnext_bwd_workspace_bytes(ops, 2, 0) == -1
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        assert lib.sdetr_convnext_bwd_run(_hip.stream_ptr(), ops, 2, 0, ws.data_ptr(), ws.numel()) != 0
        assert text in lib.sdetr_last_error().decode(), (bad, lib.sdetr_last_error())
        torch.cuda.synchronize()
        assert torch.isnan(first["out"]).all()           # the valid first op did not run


# ---- the whole network ----------------------------------------------------------------------------------------------

def _model(case, dtype=torch.float32, sd_prob=0.0, form="hip", salt=None):
    m = ConvNeXtBackbone(None, return_indices=TC.RETURN, freeze_indices=TC.FREEZE, stochastic_depth_prob=sd_prob,
                         block_setting=[CNBlockConfig(*r) for r in TC.setting(case)])
    sd = TC.state(m.state_dict(), case) if salt is None else CC.state(m.state_dict(), case, salt=salt)
    m.load_state_dict(sd)
    return m.cuda().train().set_dtype(dtype).set_train_form(form)


_canvas_cache = {}


def _canvas():
    if "x" not in _canvas_cache:
        _canvas_cache["x"] = TC.canvas().cuda()
    return _canvas_cache["x"]


def _step(m, case, cots=None):
    outs = m(_canvas())
    if cots is None:
        cots = {k: v.cuda() for k, v in TC.cotangents(case, outs).items()}
    sum((outs[k] * cots[k]).sum() for k in outs).backward()
    return cots


def _grads(m):
    return {n: p.grad for n, p in m.named_parameters() if p.requires_grad}


def _compare(gold, case, dtype, key):
    m = _model(case, dtype)
    _step(m, case)
    torch.cuda.synchronize()
    names = [str(n) for n in gold[f"{case}.names"]]
    grads = _grads(m)
    assert list(grads) == names
    assert all(p.grad is None for p in m.parameters() if not p.requires_grad)
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
        print(f"{case} {n:34s} own-scale {own:.2e} norm {rel:.2e} d_ref {d_ref:.2e} bar {bar:.2e}")
        worst = max(worst, own / bar, rel / bar)
        failures.extend((n, v, bar) for v in (own, rel) if not v <= bar)
    print(f"{case} {dtype}: worst value / bar {worst:.2f}")
    assert not failures, failures


@pytest.mark.parametrize("case", list(TC.CASES))
def test_fp32_gradients_within_the_reference_error(gold, case):
    """Every stored element and every norm within ``max(4 * d32, GRAD_FLOOR)`` of the reference's float64 gradients, on
    the tensor's own scale.  The worst ratio is printed (first MI355X run: 0.15 in both cases)."""
    _compare(gold, case, torch.float32, "d32")


@pytest.mark.parametrize("case", list(TC.CASES))
def test_bf16_gradients_within_the_reference_autocast_error(gold, case):
    """bf16 mode: bounded the same way by the reference's ``torch.autocast("cpu", bfloat16)`` distance ``dbf16``."""
    _compare(gold, case, torch.bfloat16, "dbf16")


SD_SEED = 3   # the test asserts that this seed drops at least one sample and keeps at least one


def test_stochastic_depth_draws_as_the_torch_form_and_its_gradients_match():
    case = "ct1"
    m = _model(case, sd_prob=0.5)
    seen = {}

    def hook(name, p):
        def record(mod, inp, out):
            seen[name] = (out.detach().flatten(1).abs().sum(1) > 0).float().cpu() / (1.0 - p)
        return record
    drawing = [(name, blk) for kind, name, blk in m._sequence() if kind == "block" and blk.stochastic_depth.p > 0]
    hooks = [blk.stochastic_depth.register_forward_hook(hook(name, blk.stochastic_depth.p)) for name, blk in drawing]
    m.set_train_form("torch")
    torch.manual_seed(SD_SEED)
    m(_canvas())
    for hk in hooks:
        hk.remove()
    m.set_train_form("hip")
    torch.manual_seed(SD_SEED)
    outs = m(_canvas())
    factors = {k: v.cpu() for k, v in m.stochastic_depth_factors().items()}   # (valid while the graph is alive)
    assert all(t.is_cuda for t in m.saved_activations().values())
    cots = {k: v.cuda() for k, v in TC.cotangents(case, outs).items()}
    sum((outs[k] * cots[k]).sum() for k in outs).backward()
    torch.cuda.synchronize()
    assert list(factors) == [name for name, _ in drawing]
    flat = torch.cat(list(factors.values()))
    assert (flat == 0).any() and (flat > 0).any()
    for name, f in factors.items():
        assert torch.equal(seen[name], f), (name, seen[name], f)
    # the float64 composite on the CPU under the HIP run's own factors
    ref = ConvNeXtBackbone(None, return_indices=TC.RETURN, freeze_indices=TC.FREEZE, stochastic_depth_prob=0.5,
                           block_setting=[CNBlockConfig(*r) for r in TC.setting(case)])
    ref.load_state_dict(TC.state(ref.state_dict(), case))
    ref = ref.double().train()
    for _, name, blk in ref._sequence():
        if name in factors:
            blk.stochastic_depth.forward = lambda x, f=factors[name].view(-1, 1, 1, 1): x * f.to(x.dtype)
    outs = ref.forward_torch(TC.canvas().double())
    names = [n for n, p in ref.named_parameters() if p.requires_grad]
    g64 = torch.autograd.grad(sum((outs[k] * cots[k].cpu().double()).sum() for k in outs), [dict(ref.named_parameters())[n] for n in names])
    ref.float()
    outs = ref.forward_torch(TC.canvas())
    g32 = torch.autograd.grad(sum((outs[k].double() * cots[k].cpu().double()).sum() for k in outs),
                              [dict(ref.named_parameters())[n] for n in names])
    grads, worst = _grads(m), 0.0
    for n, a, b in zip(names, g64, g32):
        scale = a.abs().max().item() or 1.0       # (a block that dropped every sample: exact zeros, held to the floor)
        d32 = (b.double() - a).abs().max().item() / scale
        own = (grads[n].cpu().double() - a).abs().max().item() / scale
        bar = max(4 * d32, GRAD_FLOOR)
        worst = max(worst, own / bar)
        assert own <= bar, (n, own, bar)
    print(f"stochastic depth: worst value / bar {worst:.2f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical_accumulation_and_graph_replay(dtype):
    case = "ct1"
    m = _model(case, dtype)
    cots = _step(m, case)
    first = {n: g.clone() for n, g in _grads(m).items()}
    _step(m, case, cots)                          # a second backward() accumulates
    torch.cuda.synchronize()
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n] + first[n]), n
    m.zero_grad(set_to_none=True)
    _step(m, case, cots)
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n]), n        # two runs, bit for bit
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _step(m, case, cots)                      # eager warm-up on the side stream
        torch.cuda.synchronize()
        for g in _grads(m).values():
            g.zero_()
        with torch.cuda.graph(graph, stream=stream):
            _step(m, case, cots)
    torch.cuda.current_stream().wait_stream(stream)
    for replay in range(2):
        for g in _grads(m).values():
            g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for n, g in _grads(m).items():
            assert torch.equal(g, first[n]), (replay, n)


def test_new_state_dict_repacks_the_backward_weights():
    case = "ct1"
    m = _model(case)
    cots = _step(m, case)
    before = {n: g.clone() for n, g in _grads(m).items()}
    m.load_state_dict(CC.state(m.state_dict(), case, salt=77))
    m.zero_grad(set_to_none=True)
    _step(m, case, cots)
    fresh = _model(case, salt=77)
    _step(fresh, case, cots)
    torch.cuda.synchronize()
    a, b = _grads(m), _grads(fresh)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert any(not torch.equal(a[n], before[n]) for n in a)


def test_hip_request_that_is_not_eligible_raises_at_forward():
    m = ConvNeXtBackbone(None, return_indices=TC.RETURN, block_setting=[CNBlockConfig(*r) for r in TC.setting("ct1")])
    m = m.cuda().set_train_form("hip")            # stem not frozen
    with pytest.raises(RuntimeError, match="stem"):
        m(_canvas())
    with pytest.raises(RuntimeError, match="float16"):
        _model("ct1", torch.float16)(_canvas())
    with pytest.raises(RuntimeError, match="input requires"):
        _model("ct1")(_canvas().clone().requires_grad_(True))


def test_detector_trains_its_convnext_backbone_in_hip():
    import test_detector_train_gpu as T
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR
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
    backbone = ConvNeXtBackbone(None, return_indices=(1, 2, 3), freeze_indices=(0,),
                                block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=T.C, num_queries=T.PROPOSALS, denoising_nums=12)
    sd = CC.syn.det_state_dict(det.state_dict(), salt=9)
    sd.update({"backbone." + k: v for k, v in CC.state(backbone.state_dict(), "cnt4").items()})
    det.load_state_dict(sd)
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
    trainable = backbone._trainable()
    assert len(trainable) > 0
    for n, p in trainable:
        g = p.grad
        assert g is not None and g.dtype == torch.float32 and g.shape == p.shape, n
        assert torch.isfinite(g).all() and g.abs().max().item() > 0, n
    assert all(p.grad is None for p in backbone.parameters() if not p.requires_grad)
    torch.cuda.synchronize()
