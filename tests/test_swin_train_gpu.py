"""GPU: training the Swin backbone in HIP (``SwinBackbone.set_train_form("hip")``, csrc/swin_backward.hip).

The two new kinds are held to float64 torch autograd, on the CPU, of this project's own modules: the window attention
backward to ``ShiftedWindowAttention`` from the qkv rows to the attention rows (its ``qkv`` replaced by a lookup of the
given rows, a token of the padding getting a bias leaf of its own, its ``proj`` by the identity), the patch-merging
backward to ``PatchMerging`` without its reduction.  fp32 bar: ``max(3 * d32, 2e-6 * scale)`` with ``d32`` the distance of
the CPU fp32 autograd run from float64, as tests/test_convnext_train_gpu.py; 16-bit bar: ``max(2e-2 * scale, 1.5 * dbf)``
with ``dbf`` the distance of the same op's CPU autograd under ``torch.autocast(bfloat16)`` from float64.  The whole-net
tests compare the parameter gradients with the imported reference's float64 gradients (tests/golden/swin_train.npz)
against the reference's own fp32 / bf16-autocast error.  Every test prints its worst value / bar; first MI355X run:
attention backward fp32 0.22 (dqkv) / 0.09 (padded bias) / 0.18 (table), bf16 0.24 / 0.04 / < 0.001; merging backward
0.09; whole net fp32 0.23 / 0.27 / 0.21 and bf16 0.24 / 0.31 / 0.35 (w7t / w12t / lt); stochastic depth 0.28."""
import numpy as np
import pytest
import torch
from torch import nn

import swin_cases as SC
import swin_train_cases as TC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.swin import PatchMerging, ShiftedWindowAttention, SwinBackbone

pytestmark = pytest.mark.gpu
GRAD_FLOOR = 5e-6   # as tests/test_backbone_train_gpu.py
B = 2


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TC.GOLDEN))


def _act(precision):
    return torch.float32 if precision == 0 else torch.bfloat16


def _op(**fields):
    return _hip.SwinBwdOpStruct(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in fields.items()})


def _run(precision, **fields):
    """One ``sdetr_swin_bwd_op_run``; tensors in ``fields`` become their pointers."""
    lib = _hip.lib()
    op = (_hip.SwinBwdOpStruct * 1)(_op(**fields))
    nbytes = lib.sdetr_swin_bwd_workspace_bytes(op, 1, precision)
    _hip.check(0 if nbytes >= 0 else -1, "swin bwd workspace", lib)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_swin_bwd_op_run(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "swin bwd op", lib)
    torch.cuda.synchronize()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")   # every element must be written


def _check(what, got, r64, r32, rbf, precision, worst):
    scale = r64.abs().max().item()
    err = (got.detach().cpu().double() - r64).abs().max().item()
    if precision == 0:
        bar = max(3 * (r32.double() - r64).abs().max().item(), 2e-6 * scale)
    else:
        bar = max(2e-2 * scale, 1.5 * (rbf.double() - r64).abs().max().item())
    if bar == 0.0:                                        # an all-zero reference (no padding): exact zeros
        assert err == 0.0, (what, err)
        return
    worst[what] = max(worst.get(what, 0.0), err / bar)
    assert torch.isfinite(got).all() and err <= bar, (what, err, bar, scale)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class _Rows(nn.Module):
    """Stands in for ``attn.qkv``: channel 0 of a token is its row + 1 (0 on the zero padding); returns that row of the
    given qkv rows, or the padding's own bias leaf."""

    def __init__(self, rows, pad):
        super().__init__()
        self.rows, self.pad = rows, pad

    def forward(self, tokens):
        return torch.cat([self.pad[None].to(self.rows.dtype), self.rows])[tokens[..., 0].round().long()]


def _attention_grads(attn, qkv, bias, dout, h, w, dtype, autocast=None):
    c = dout.shape[-1]
    a = ShiftedWindowAttention(c, attn.window_size, attn.shift_size, attn.num_heads).to(dtype)
    a.relative_position_bias_table.data.copy_(attn.relative_position_bias_table.data)
    rows = qkv.reshape(-1, 3 * c).to(dtype).requires_grad_(True)
    pad = bias.to(dtype).requires_grad_(True)
    a.qkv, a.proj = _Rows(rows, pad), nn.Identity()
    x = torch.zeros(B, h, w, c, dtype=dtype)
    x[..., 0] = torch.arange(1, B * h * w + 1, dtype=dtype).view(B, h, w)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            out = a(x)
    else:
        out = a(x)
    g = torch.autograd.grad((out.double() * dout.double()).sum(), (rows, pad, a.relative_position_bias_table))
    return [t.double() for t in g]


ATTENTION = [(7, 12, 30, 3, 3), (7, 6, 15, 3, 3), (7, 2, 4, 3, 6), (7, 14, 14, 0, 3), (12, 25, 37, 6, 2), (12, 13, 19, 6, 4)]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", ATTENTION)
def test_window_attention_backward_kind(shape, precision):
    window, h, w, shift, heads = shape
    c, act, worst = 32 * heads, _act(precision), {}
    attn = ShiftedWindowAttention(c, (window, window), (shift, shift), heads)
    attn.relative_position_bias_table.data = _rand(1, *attn.relative_position_bias_table.shape)
    qkv = _rand(2, B, h, w, 3 * c).to(act).float()
    bias = (0.5 * _rand(3, 3 * c)).to(torch.bfloat16).float()
    dout = _rand(4, B, h, w, c).to(act).float()
    r64 = _attention_grads(attn, qkv, bias, dout, h, w, torch.float64)
    r32 = _attention_grads(attn, qkv, bias, dout, h, w, torch.float32)
    rbf = _attention_grads(attn, qkv, bias, dout, h, w, torch.float32, torch.bfloat16) if precision else r32
    index = attn.relative_position_index.reshape(-1)
    entries = attn.relative_position_bias_table.shape[0]
    order = torch.argsort(index, stable=True).to(torch.int32).cuda()
    offsets = torch.zeros(entries + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.bincount(index, minlength=entries), 0)
    offsets = offsets.to(torch.int32).cuda()
    dqkv, dpad, dtable = _nan((B, h, w, 3 * c), act), _nan((3 * c,)), _nan((entries, heads))
    with torch.no_grad():
        table = attn.position_bias().float().contiguous().cuda()
    _run(precision, kind=6, x=qkv.to(act).cuda(), dz=dout.to(act).cuda(), bias=bias.cuda(), table=table, order=order,
         offsets=offsets, out=dqkv, dbias=dpad, dtable=dtable, batch=B, channels=c, height=h, width=w, window=window,
         shift=shift, heads=heads)
    _check("dqkv", dqkv.float().reshape(-1, 3 * c), r64[0], r32[0], rbf[0], precision, worst)
    _check("padded bias", dpad, r64[1], r32[1], rbf[1], precision, worst)
    _check("table", dtable, r64[2], r32[2], rbf[2], precision, worst)
    padded = h % window != 0 or w % window != 0
    assert (r64[1].abs().max().item() > 0) == padded
    if padded:   # dropping the padded tokens' share of the qkv bias gradient fails here
        assert dpad[c:].abs().max().item() > 0.1 * r64[1].abs().max().item() and (dpad[:c] == 0).all()
    else:
        assert (dpad == 0).all()
    print(shape, precision, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("shape", [(96, 5, 7), (96, 6, 8), (768, 5, 7)])
def test_patch_merging_backward_kind(shape, precision):
    c, h, w = shape
    act, worst = _act(precision), {}
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x = _rand(5, B, h, w, c) * 1.5 + 0.3
    dz = _rand(6, B, ho, wo, 4 * c).to(act).float()
    gamma, add = 1 + 0.2 * _rand(7, 4 * c), _rand(8, B, h, w, c)

    def grads(dt, autocast=None):
        m = PatchMerging(c, lambda n: nn.LayerNorm(n, eps=1e-5)).to(dt)
        m.reduction = nn.Identity()
        m.norm.weight.data.copy_(gamma)
        xx = x.to(dt).requires_grad_(True)
        if autocast is not None:
            with torch.autocast("cpu", dtype=autocast):
                y = m(xx)
        else:
            y = m(xx)
        return [t.double() for t in torch.autograd.grad((y.double() * dz.double()).sum(), (xx, m.norm.weight, m.norm.bias))]
    r64, r32 = grads(torch.float64), grads(torch.float32)
    rbf = grads(torch.float32, torch.bfloat16) if precision else r32
    for with_add in (True, False):
        out, dg, db = _nan((B, h, w, c)), _nan((4 * c,)), _nan((4 * c,))
        _run(precision, kind=8, dz=dz.to(act).cuda(), x=x.cuda(), gamma=gamma.cuda(), add=add.cuda() if with_add else None, out=out,
             dgamma=dg, dbeta=db, batch=B, channels=c, height=h, width=w, eps=1e-5)
        # the stream gradient and the affine gradients are fp32 in both precisions: only dz is 16-bit, and the
        # reference sees the same rounded dz
        _check("merge dx", out.cpu() - add if with_add else out, r64[0], r32[0], rbf[0], 0, worst)
        _check("merge dgamma", dg, r64[1], r32[1], rbf[1], 0, worst)
        _check("merge dbeta", db, r64[2], r32[2], rbf[2], 0, worst)
    print(shape, precision, {k: round(v, 3) for k, v in worst.items()})


def test_a_bad_backward_op_is_rejected_before_any_launch():
    lib = _hip.lib()
    c, h, w, heads = 96, 5, 7, 3
    t = torch.zeros(B * h * w * 3 * c + 4096, device="cuda")
    idx = torch.zeros(4096, dtype=torch.int32, device="cuda")
    good = dict(kind=6, x=t, dz=t[16:], bias=t, table=t, order=idx, offsets=idx, out=t[32:], dbias=t, dtable=t, batch=B, channels=c,
                height=h, width=w, window=7, shift=3, heads=heads)
    for bad, text in ((dict(x=None), "null"), (dict(window=8), "window"), (dict(heads=2), "head dimension"), (dict(), "workspace")):
        first = dict(kind=5, dz=t, out=_nan((B, h, w, c)), batch=B, channels=c, height=h, width=w)
        ops = (_hip.SwinBwdOpStruct * 2)(_op(**first), _op(**{**good, **bad}))
        need = lib.sdetr_swin_bwd_workspace_bytes(ops, 2, 0)
        ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
        if bad:
            assert need == -1
            rc = lib.sdetr_swin_bwd_run(_hip.stream_ptr(), ops, 2, 0, ws.data_ptr(), ws.numel())
        else:            # a valid plan over a workspace that is too small
            assert 16 < need <= ws.numel()
            rc = lib.sdetr_swin_bwd_run(_hip.stream_ptr(), ops, 2, 0, ws.data_ptr(), need - 16)
        assert rc == _hip.EINVAL
        assert text in lib.sdetr_last_error().decode(), (bad, lib.sdetr_last_error())
        torch.cuda.synchronize()
        assert torch.isnan(first["out"]).all()           # the valid first op did not run


# ---- the whole network ----------------------------------------------------------------------------------------------

def _model(case, dtype=torch.float32, sd_prob=0.0, form="hip", salt=None, **kw):
    m = SwinBackbone(None, return_indices=TC.RETURN, freeze_indices=kw.pop("freeze_indices", TC.FREEZE),
                     **TC.config(case, sd_prob), **kw)
    m.load_state_dict(TC.state(m.state_dict(), case, salt=salt))
    return m.cuda().train().set_dtype(dtype).set_train_form(form)


_canvas_cache = {}


def _canvas(case):
    if case not in _canvas_cache:
        _canvas_cache[case] = TC.canvas(case).cuda()
    return _canvas_cache[case]


def _step(m, case, cots=None):
    outs = m(_canvas(case))
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
        print(f"{case} {n:52s} own-scale {own:.2e} norm {rel:.2e} d_ref {d_ref:.2e} bar {bar:.2e}")
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


SD_SEED = 3   # the test asserts that this seed drops at least one sample and keeps at least one


def test_stochastic_depth_draws_as_the_torch_form_and_its_gradients_match():
    case = "w7t"
    m = _model(case, sd_prob=0.5)
    seen = {}

    def hook(name, p):
        def record(mod, inp, out):
            branch = ".attn" if name + ".attn" not in seen else ".mlp"
            seen[name + branch] = (out.detach().flatten(1).abs().sum(1) > 0).float().cpu() / (1.0 - p)
        return record
    drawing = [(name, blk) for kind, name, blk in m._sequence() if kind == "block" and blk.stochastic_depth.p > 0]
    hooks = [blk.stochastic_depth.register_forward_hook(hook(name, blk.stochastic_depth.p)) for name, blk in drawing]
    m.set_train_form("torch")
    torch.manual_seed(SD_SEED)
    m(_canvas(case))
    for hk in hooks:
        hk.remove()
    m.set_train_form("hip")
    torch.manual_seed(SD_SEED)
    outs = m(_canvas(case))
    factors = {k: v.cpu() for k, v in m.stochastic_depth_factors().items()}   # (valid while the graph is alive)
    assert all(t.is_cuda for t in m.saved_activations().values())
    cots = {k: v.cuda() for k, v in TC.cotangents(case, outs).items()}
    sum((outs[k] * cots[k]).sum() for k in outs).backward()
    torch.cuda.synchronize()
    assert list(factors) == [name + branch for name, _ in drawing for branch in (".attn", ".mlp")]   # two per block
    flat = torch.cat(list(factors.values()))
    assert (flat == 0).any() and (flat > 0).any()
    for name, f in factors.items():
        assert torch.equal(seen[name], f), (name, seen[name], f)
    # the float64 composite on the CPU under the HIP run's own factors
    ref = SwinBackbone(None, return_indices=TC.RETURN, freeze_indices=TC.FREEZE, **TC.config(case, 0.5))
    ref.load_state_dict(TC.state(ref.state_dict(), case))
    ref = ref.double().train()
    names = [n for n, p in ref.named_parameters() if p.requires_grad]

    def run(x):
        for _, name, blk in ref._sequence():
            if name + ".attn" in factors:
                pair = [factors[name + ".attn"].view(-1, 1, 1, 1), factors[name + ".mlp"].view(-1, 1, 1, 1)]
                blk.stochastic_depth.forward = lambda t, q=pair: t * q.pop(0).to(t.dtype)
        outs_ = ref.forward_torch(x)
        return torch.autograd.grad(sum((outs_[k].double() * cots[k].cpu().double()).sum() for k in outs_),
                                   [dict(ref.named_parameters())[n] for n in names])
    g64 = run(TC.canvas(case).double())
    ref.float()
    g32 = run(TC.canvas(case))
    grads, worst = _grads(m), 0.0
    for n, a, b in zip(names, g64, g32):
        scale = a.abs().max().item() or 1.0       # (a branch that dropped every sample: exact zeros, held to the floor)
        d32 = (b.double() - a).abs().max().item() / scale
        own = (grads[n].cpu().double() - a).abs().max().item() / scale
        bar = max(4 * d32, GRAD_FLOOR)
        worst = max(worst, own / bar)
        assert own <= bar, (n, own, bar)
    print(f"stochastic depth: worst value / bar {worst:.2f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_bit_identical_accumulation_and_graph_replay(dtype):
    case = "w7t"
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


def test_new_state_dict_repacks_the_backward_operands_and_the_table():
    case = "w7t"
    m = _model(case)
    cots = _step(m, case)
    before = {n: g.clone() for n, g in _grads(m).items()}
    m.load_state_dict(TC.state(m.state_dict(), case, salt=77))
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
    case = "w7t"
    with pytest.raises(RuntimeError, match="no HIP backward"):
        _model(case, freeze_indices=())(_canvas(case))   # stem not frozen
    with pytest.raises(RuntimeError, match="float16"):
        _model(case, torch.float16)(_canvas(case))
    with pytest.raises(RuntimeError, match="input requires"):
        _model(case)(_canvas(case).clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="dropout"):
        _model(case, dropout=0.1)(_canvas(case))


def test_detector_trains_its_swin_backbone_in_hip():
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
    backbone = SwinBackbone(None, return_indices=(1, 2, 3), freeze_indices=(0,), embed_dim=32, depths=(1, 2, 2, 1),
                            num_heads=(1, 2, 4, 8), window_size=(7, 7), stochastic_depth_prob=0.0)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=T.C, num_queries=T.PROPOSALS, denoising_nums=12)
    sd = SC.syn.det_state_dict(det.state_dict(), salt=9)
    sd.update({"backbone." + k: v for k, v in SC.state(backbone.state_dict(), "det").items()})
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
