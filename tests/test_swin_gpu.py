"""GPU: the Swin backbone (csrc/swin.hip): the window attention, the patch-merging gather + LayerNorm, the qkv epilogue
into the compute dtype, and ``SwinBackbone``.

Each op against a float64 torch statement of its ABI contract.  The attention statement is written from the reference
function's definition on the op's inputs (pad with the bias, roll, windows, scores + table + the mask from the reference's
slices, softmax, product, reverse): fp32 ``err <= max(2 d_torch32, 1e-6 max|ref|)`` with ``d_torch32`` the same statement
in fp32; in 16-bit the operands are pre-rounded and ``err <= 2 d_torch16``, the same statement run in the 16-bit dtype on
the CPU.  The merging is held to the FocalNet LayerNorm bound (2^-8 / 2^-11 ``|ref|`` more in 16-bit), the qkv GEMM to
2e-6 / 2e-2 of ``max|ref|`` with a pre-rounded A operand.  The module against the imported reference
(tests/golden/swin_cases.npz, make_swin_golden.py) in fp32 and under the reference's own autocast distance in bf16 /
fp16; run-to-run and graph-replay bit equality; the ``derived`` key after ``load_state_dict``; 16-bit parameters; the
composite under grad; the detector from images.

Whole network, worst d / bound over the returned stages (first GPU run, one MI355X; also DESIGN.md §4 "Swin backbone"):
fp32 0.08 (l stage 3; w12 0.07, w7 0.06); bf16 0.45 (w7 stage 3; w12 0.45, l 0.42); fp16 0.52 (w7 stage 2; l 0.48,
w12 0.42)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_cases as SC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.backbone import batch_images
from salience_detr_amd.swin import SwinBackbone

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_cases.npz")
ACT = {torch.float32: (0, None), torch.bfloat16: (1, 2.0 ** -8), torch.float16: (1, 2.0 ** -11)}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, dtype=torch.float32, salt=None, ret=None):
    m = SwinBackbone(None, return_indices=ret or SC.CASES[name][1], **SC.config(name))
    m.load_state_dict(SC.state(m.state_dict(), name, salt))
    return m.eval().cuda().set_dtype(dtype)


def _run(m, x):
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    return out


def _lib(dtype):
    return _hip.lib(dtype if dtype == torch.float16 else None)


def _ptr(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def _op(lib, precision, **kw):
    base = dict(kind=0, x=None, weight=None, bias=None, gamma=None, beta=None, residual=None, table=None, out=None,
                out_nchw=None, batch=1, in_channels=32, height=1, width=1, out_channels=32, kernel_size=1, stride=1, x_nchw=0,
                out_f32=0, window=0, shift=0, heads=0, splits=0, eps=1e-5)
    base.update({k: _ptr(v) for k, v in kw.items()})
    arr = (_hip.SwinOpStruct * 1)(_hip.SwinOpStruct(**base))
    nbytes = lib.sdetr_swin_workspace_bytes(arr, 1, precision)
    assert nbytes >= 0, lib.sdetr_last_error().decode()
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.launch("sdetr_swin_op_run", lib, ws.device, arr, precision, ws.data_ptr(), ws.numel(), what="swin op")
    torch.cuda.synchronize()
    return nbytes


def _check(what, got, ref, t32, rounding=None):
    """fp32: max err <= max(2 d_torch32, 1e-6 max|ref|); 16-bit: elementwise, ``rounding * |ref|`` more."""
    d32 = (t32.double() - ref).abs().max().item()
    bound = max(2 * d32, 1e-6 * ref.abs().max().item())
    err = (got.double().cpu() - ref).abs()
    print(f"{what}: d {err.max().item():.3g} d_torch32 {d32:.3g} bound {bound:.3g}")
    if rounding is None:
        assert err.max().item() <= bound, (what, err.max().item(), bound)
    else:
        assert bool((err <= bound + rounding * ref.abs()).all()), (what, (err - rounding * ref.abs()).max().item(), bound)


# ---- window attention against its ABI contract ---------------------------------------------------------------------

def _attention_statement(qkv, bias, table, window, shift, heads, dt, zero_padding=False):
    """``qkv`` ``[B, H, W, 3 C]`` (the bias already inside), ``bias`` ``[3 C]``, ``table`` ``[heads, N, N]`` -> ``[B, H, W, C]``
    in ``dt``.  ``zero_padding``: the WRONG variant in which a token of the padding has q = k = v = 0."""
    B, H, W, C3 = qkv.shape
    C, n = C3 // 3, window * window
    ph, pw = -(-H // window) * window, -(-W // window) * window
    full = (torch.zeros(C3) if zero_padding else bias).to(dt).expand(B, ph, pw, C3).clone()
    full[:, :H, :W] = qkv.to(dt)
    s = [0 if window >= ph else shift, 0 if window >= pw else shift]
    if sum(s) > 0:
        full = torch.roll(full, shifts=(-s[0], -s[1]), dims=(1, 2))
    nh, nw = ph // window, pw // window
    t = full.view(B, nh, window, nw, window, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nh * nw, n, 3, heads, C // heads)
    q, k, v = t.permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q * (C // heads) ** -0.5).matmul(k.transpose(-2, -1)) + table.to(dt).unsqueeze(0)
    if sum(s) > 0:
        ids = torch.zeros(ph, pw)
        count = 0
        for hs in ((0, -window), (-window, -s[0]), (-s[0], None)):
            for ws_ in ((0, -window), (-window, -s[1]), (-s[1], None)):
                ids[hs[0]:hs[1], ws_[0]:ws_[1]] = count
                count += 1
        ids = ids.view(nh, window, nw, window).permute(0, 2, 1, 3).reshape(nh * nw, n)
        diff = ids.unsqueeze(1) - ids.unsqueeze(2)
        mask = torch.where(diff != 0, -100.0, 0.0).to(dt)
        attn = (attn.view(B, nh * nw, heads, n, n) + mask[None, :, None]).view(-1, heads, n, n)
    out = F.softmax(attn, dim=-1).matmul(v).transpose(1, 2).reshape(B, nh, nw, window, window, C)
    out = out.permute(0, 1, 3, 2, 4, 5).reshape(B, ph, pw, C)
    if sum(s) > 0:
        out = torch.roll(out, shifts=(s[0], s[1]), dims=(1, 2))
    return out[:, :H, :W].contiguous()


def _attention_inputs(H, W, window, heads, dtype, bias_scale, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    C = 32 * heads
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    bias = bias_scale * torch.randn(3 * C, generator=g)
    table = 2 * torch.rand(heads, window * window, window * window, generator=g) - 1
    if dtype != torch.float32:
        qkv, bias = qkv.to(dtype).float(), bias.to(dtype).float()
    return qkv, bias, table


def _attention_hip(qkv, bias, table, window, shift, heads, dtype):
    B, H, W, C3 = qkv.shape
    out = torch.full((B, H, W, C3 // 3), float("nan"), dtype=dtype, device="cuda")
    _op(_lib(dtype), ACT[dtype][0], kind=4, x=qkv.to(dtype).cuda(), bias=bias.cuda(), table=table.contiguous().cuda(), out=out,
        batch=B, in_channels=C3 // 3, height=H, width=W, out_channels=C3 // 3, window=window, shift=shift, heads=heads)
    return out


def _attention_bound(args, dtype, ref):
    if dtype == torch.float32:
        return max(2 * (_attention_statement(*args, torch.float32).double() - ref).abs().max().item(),
                   1e-6 * ref.abs().max().item())
    return 2 * (_attention_statement(*args, dtype).double() - ref).abs().max().item()


ATTENTION_SHAPES = [   # (H, W, window, shift, heads)
    (12, 30, 7, 3, 3),      # pads to 14 x 35: shift on both axes, both paddings
    (6, 15, 7, 3, 3),       # pads to 7 x 21: the row shift switches off
    (2, 4, 7, 3, 3),        # pads to 7 x 7: no shift, one window, 41 of its 49 tokens are padding
    (25, 37, 12, 6, 2),     # 144-token windows, pads to 36 x 48
    (14, 21, 7, 0, 3),      # exactly divisible
    (14, 21, 7, 3, 3),
    (2, 3, 7, 3, 48),       # the last stage of swin_l
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ATTENTION_SHAPES)
def test_window_attention_contract(shape, dtype):
    H, W, window, shift, heads = shape
    qkv, bias, table = _attention_inputs(H, W, window, heads, dtype, 0.3, H * 100 + W + shift)
    args = (qkv, bias, table, window, shift, heads)
    ref = _attention_statement(*args, torch.float64)
    bound = _attention_bound(args, dtype, ref)
    got = _attention_hip(*args, dtype)
    d = (got.double().cpu() - ref).abs().max().item()
    print(f"attention {shape} {dtype}: d {d:.3g} bound {bound:.3g} d / bound {d / bound:.3f}")
    assert d <= bound, (shape, d, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_tokens_are_live_keys(dtype):
    H, W, window, shift, heads = 6, 15, 7, 3, 3
    qkv, bias, table = _attention_inputs(H, W, window, heads, dtype, 1.0, 77)
    args = (qkv, bias, table, window, shift, heads)
    ref = _attention_statement(*args, torch.float64)
    bound = _attention_bound(args, dtype, ref)
    wrong = (_attention_statement(*args, torch.float64, zero_padding=True) - ref).abs().max().item()
    assert wrong > bound, (wrong, bound)             # the bound tells the two variants apart
    d = (_attention_hip(*args, dtype).double().cpu() - ref).abs().max().item()
    print(f"padded tokens {dtype}: d {d:.3g} bound {bound:.3g} zero-padding variant {wrong:.3g}")
    assert d <= bound, (d, bound)


# ---- patch merging and the qkv epilogue ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(6, 15), (3, 8), (4, 6)])           # odd W, odd H, both even
@pytest.mark.parametrize("C", [96, 768])
def test_patch_merging_contract(C, hw, dtype):
    precision, rounding = ACT[dtype]
    (H, W), B = hw, 2
    g = torch.Generator().manual_seed(C + H)
    x = 3 * torch.randn(B, H, W, C, generator=g) + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(4 * C, generator=g), 0.1 * torch.randn(4 * C, generator=g)

    def statement(dt):
        p = F.pad(x.to(dt), (0, 0, 0, W % 2, 0, H % 2))
        cat = torch.cat([p[:, 0::2, 0::2], p[:, 1::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 1::2]], -1)
        return F.layer_norm(cat, (4 * C,), gamma.to(dt), beta.to(dt), 1e-5)
    out = torch.full((B, (H + 1) // 2, (W + 1) // 2, 4 * C), float("nan"), dtype=dtype, device="cuda")
    _op(_lib(dtype), precision, kind=5, x=x.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), out=out, batch=B, in_channels=C,
        height=H, width=W, out_channels=4 * C)
    _check(f"merging C={C} {hw} {dtype}", out, statement(torch.float64), statement(torch.float32), rounding)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [32, 96, 1536, 3072])          # 32: 8 lanes own a quad; 3072: all 12 quads of every lane
def test_layer_norm_contract(C, dtype):
    precision, rounding = ACT[dtype]
    g = torch.Generator().manual_seed(C)
    x = 3 * torch.randn(2, 5, 7, C, generator=g) + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    statement = lambda dt: F.layer_norm(x.to(dt), (C,), gamma.to(dt), beta.to(dt), 1e-5)
    for out_f32 in (0, 1):
        out = torch.full((2, 5, 7, C), float("nan"), dtype=torch.float32 if out_f32 else dtype, device="cuda")
        _op(_lib(dtype), precision, kind=3, x=x.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), out=out, batch=2, in_channels=C,
            height=5, width=7, out_channels=C, out_f32=out_f32)
        _check(f"ln C={C} {dtype} f32={out_f32}", out, statement(torch.float64), statement(torch.float32),
               None if out_f32 else rounding)


def _pack(lib, w, bias, precision):
    co, ci = w.shape
    f32 = [t.float().contiguous().cuda() for t in (w, torch.ones(co), bias, torch.zeros(co), torch.ones(co))]
    packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, 1, precision) // 2, dtype=torch.int16, device="cuda")
    out_bias = torch.empty(co, device="cuda")
    _hip.launch("sdetr_backbone_pack", lib, packed.device, *[t.data_ptr() for t in f32], 0.0, co, ci, 1, 0, precision,
                packed.data_ptr(), out_bias.data_ptr())
    return packed, out_bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("C", [96, 1536])
def test_linear_into_the_compute_dtype_contract(C, splits, dtype):
    precision, _ = ACT[dtype]
    lib, B, H, W = _lib(dtype), 2, 9, 15                            # 270 rows: two row tiles, the second ragged
    g = torch.Generator().manual_seed(C + splits)
    a = torch.randn(B, H, W, C, generator=g)
    w, bias = torch.randn(3 * C, C, generator=g) / C ** 0.5, 0.1 * torch.randn(3 * C, generator=g)
    if precision == 1:
        a = a.to(dtype).float()
    ref = F.linear(a.double(), w.double(), bias.double())
    packed, pbias = _pack(lib, w, bias, precision)
    out = torch.full((B, H, W, 3 * C), float("nan"), dtype=dtype, device="cuda")
    nbytes = _op(lib, precision, kind=2, x=a.to(dtype).cuda(), weight=packed, bias=pbias, out=out, batch=B, in_channels=C,
                 height=H, width=W, out_channels=3 * C, splits=splits)
    if splits > 1:
        assert nbytes == splits * B * H * W * 3 * C * 4
    d = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"qkv C={C} splits={splits} {dtype}: d / scale {d:.3g}")
    assert d <= (2e-6 if precision == 0 else 2e-2)


# ---- the module against the imported reference --------------------------------------------------------------------

def _picked(t, ref):
    flat = t.reshape(-1).double().cpu()
    return flat if ref.size == flat.numel() else flat[SC.sub_index(flat.numel())]


@pytest.mark.parametrize("name", list(SC.CASES))
def test_swin_fp32_matches_reference(gold, name):
    out = _run(_model(name), SC.canvas(name).cuda())
    assert list(out) == [f"features.{2 * i + 1}" for i in SC.CASES[name][1]]
    for key, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous()
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        print(f"{name} fp32 {key}: d / bound {d / bound:.3f}")
        assert d <= bound, (key, d, bound)


@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_swin_16bit_within_reference_autocast(gold, name, dtype, tag):
    out = _run(_model(name, dtype), SC.canvas(name).cuda())
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = 1.5 * gold[f"{name}.d{tag}_{key}"]
        print(f"{name} {tag} {key}: d / bound {d / bound:.3f}")
        assert d <= bound, (key, d, bound)


# ---- determinism, graphs, caches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_and_graph_replay_bit_identical(dtype):
    m, x = _model("w7", dtype), SC.canvas("w7").cuda()
    with torch.no_grad():
        a = {k: v.clone() for k, v in m(x).items()}
        b = m(x)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k])
        graph = graph_guard.new_graph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            m(x)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                out = m(x)
        torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], out[k])


def test_load_state_dict_and_in_place_edits_repack():
    x = SC.canvas("w12").cuda()
    m = _model("w12")
    _run(m, x)                                     # packs the first weight set
    other = _model("w12", salt=99)
    m.load_state_dict(other.state_dict())
    a, b = _run(m, x), _run(other, x)
    for k in a:
        assert torch.equal(a[k], b[k])
    a = {k: v.clone() for k, v in a.items()}
    with torch.no_grad():                          # an in-place edit of the bias table expands it again
        m.body.features[1][0].attn.relative_position_bias_table.mul_(-1.0)
    c = _run(m, x)
    assert not torch.equal(c["features.1"], a["features.1"])


def test_16bit_parameters_compute_as_their_fp32_values():
    x = SC.canvas("w7").cuda()
    m16 = _model("w7").to(torch.bfloat16)
    m32 = _model("w7")
    m32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in m16.state_dict().items()})
    a, b = _run(m16, x), _run(m32, x)
    for k in a:
        assert torch.equal(a[k], b[k])


@pytest.mark.parametrize("name", ["w7", "w12"])
def test_composite_under_grad(name):
    m, x = _model(name), SC.canvas(name).cuda()
    out = m(x)                                     # grad enabled, parameters require grad
    with torch.no_grad():
        hip = m(x)
    for k in out:
        assert out[k].grad_fn is not None
        assert (hip[k] - out[k]).abs().max().item() <= 1e-4 * out[k].abs().max().item()
    sum(v.square().mean() for v in out.values()).backward()
    grad = m.body.features[1][1].attn.relative_position_bias_table.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and grad.abs().max().item() > 0


# ---- the detector from images --------------------------------------------------------------------------------------

def test_salience_detr_with_a_swin_backbone_equals_chain_by_hand():
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR, SalienceDETRHead
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    cfg = dict(SC.config("w7"), embed_dim=64, num_heads=(2, 4, 8, 16))
    backbone = SwinBackbone(None, return_indices=(1, 2, 3), **cfg)
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(50))
    sd = SC.syn.det_state_dict(det.state_dict(), salt=5)
    sd.update({"backbone." + k: v for k, v in SC.state(backbone.state_dict(), "w7").items()})
    det.load_state_dict(sd)
    det = det.eval().cuda()
    sizes = [(160, 224), (150, 200)]
    imgs = [SC.syn.det_rand(f"detector.img{i}", (3, h, w)).cuda() for i, (h, w) in enumerate(sizes)]
    got = det(imgs)
    with torch.no_grad():
        canvas, mask = batch_images(imgs)
        feats = det.backbone(canvas)
        want = SalienceDETRHead.forward(det, feats, mask, torch.tensor(sizes, device="cuda"),
                                        image_sizes=[list(s) for s in sizes], canvas=tuple(canvas.shape[-2:]))
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert a["scores"].numel() > 0
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(a[k], b[k]), k
