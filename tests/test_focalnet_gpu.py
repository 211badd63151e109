"""GPU: the FocalNet backbone (csrc/focalnet.hip): the focal level, the modulator finish, ``h`` with the ``* q`` epilogue,
the LayerNorm variants, the patch embeddings with their ceil output size, and ``FocalNetBackbone``.

Each op against a float64 torch statement of its ABI contract (fp32 outputs: ``err <= max(2 d_torch32, 1e-6 max|ref|)``
with ``d_torch32`` torch's own fp32 distance on the same inputs; 16-bit outputs 2^-8 / 2^-11 ``|ref|`` more; GEMMs 2e-6 /
2e-2 of ``max|ref|`` with pre-rounded 16-bit A operands); the module against the imported reference
(tests/golden/focalnet_cases.npz, make_focalnet_golden.py) in fp32 and under the reference's own autocast distance in
bf16 / fp16; run-to-run and graph-replay bit equality; the ``derived`` key after ``load_state_dict``; 16-bit parameters;
the composite under grad; the detector from images.

Whole network, worst d / bound over the returned stages (first GPU run, one MI355X; also DESIGN.md §4 "FocalNet
backbone"): fp32 0.12 (srf stage 2; fl4 0.07, hg 0.05); bf16 0.56 (hg stage 3; fl4 0.55, srf 0.53); fp16 0.55 (srf stage 0;
fl4 0.52, hg 0.47)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focalnet_cases as FC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.backbone import batch_images
from salience_detr_amd.focalnet import FocalNetBackbone

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focalnet_cases.npz")
ACT = {torch.float32: (0, None), torch.bfloat16: (1, 2.0 ** -8), torch.float16: (1, 2.0 ** -11)}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, dtype=torch.float32, salt=None, ret=None):
    m = FocalNetBackbone(None, return_indices=ret or FC.CASES[name][1], **FC.config(name))
    m.load_state_dict(FC.state(m.state_dict(), name, salt))
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


def _op(lib, precision, ws=None, **kw):
    """Run one op; returns its workspace (so that a finish can read what the last level left)."""
    base = dict(kind=0, x=None, weight=None, bias=None, gamma=None, beta=None, residual=None, q=None, out=None, out2=None,
                batch=1, in_channels=32, height=1, width=1, out_channels=32, out_height=1, out_width=1, kernel_size=1,
                stride=1, padding=0, x_nchw=0, out_f32=0, x_ld=0, q_ld=0, accumulate=0, last=0, splits=0, eps=1e-5)
    base.update({k: _ptr(v) for k, v in kw.items()})
    arr = (_hip.FocalnetOpStruct * 1)(_hip.FocalnetOpStruct(**base))
    nbytes = lib.sdetr_focalnet_workspace_bytes(arr, 1, precision)
    assert nbytes >= 0, lib.sdetr_last_error().decode()
    if ws is None:
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= nbytes
    _hip.launch("sdetr_focalnet_op_run", lib, ws.device, arr, precision, ws.data_ptr(), ws.numel(), what="focalnet op")
    torch.cuda.synchronize()
    return ws, nbytes


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


# ---- ops against their ABI contract --------------------------------------------------------------------------------

def _rows(t):
    """NCHW -> channels-last rows."""
    return t.permute(0, 2, 3, 1).contiguous()


def _level_inputs(C, H, W, k, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    ld = (2 * C + 2 + 31) // 32 * 32
    frow = torch.randn(B, H, W, ld, generator=g)                    # [q | ctx | gate 0, gate 1 | padding]
    w = torch.randn(C, 1, k, k, generator=g) / k
    return frow, w, ld


def _level_ref(frow, w, C, k, dt):
    ctx = frow[..., C:2 * C].permute(0, 3, 1, 2).to(dt)
    return F.gelu(F.conv2d(ctx, w.to(dt), padding=k // 2, groups=C))    # NCHW


def _tile_sums(t):
    """[B, C, H, W] -> [B, tiles, C]: sums over the level kernel's 8 (wide) x 16 (tall) pixel tiles, row-major tiles."""
    B, C, H, W = t.shape
    return torch.stack([t[:, :, y:y + 16, x:x + 8].sum((2, 3)) for y in range(0, H, 16) for x in range(0, W, 8)], 1)


@pytest.mark.parametrize("hw", [(9, 13), (20, 23)])
@pytest.mark.parametrize("C", [96, 192, 1536])
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_focal_level_contract(k, C, hw):
    lib, (H, W), B = _hip.lib(), hw, 2
    frow, w, ld = _level_inputs(C, H, W, k, 1000 * k + C + H)
    ref, t32 = _level_ref(frow, w, C, k, torch.float64), _level_ref(frow, w, C, k, torch.float32)
    gate = frow[..., 2 * C:2 * C + 2].permute(0, 3, 1, 2)
    fd, taps = frow.cuda(), w.reshape(C, k * k).t().contiguous().cuda()
    ctx = torch.empty(B, H, W, C, device="cuda")
    total = torch.empty(B, H, W, C, device="cuda")
    common = dict(kind=3, x=fd.data_ptr() + 4 * C, weight=taps, batch=B, in_channels=C, height=H, width=W, out_channels=C,
                  kernel_size=k, x_ld=ld, q_ld=ld)
    # the first level writes ctx_all ...
    _op(lib, 0, q=fd.data_ptr() + 4 * 2 * C, out=ctx, out2=total, **common)
    _check(f"level k={k} C={C} {hw} ctx", ctx.permute(0, 3, 1, 2), ref, t32)
    _check("  ctx_all (write)", total.permute(0, 3, 1, 2), ref * gate[:, :1].double(), t32 * gate[:, :1])
    # ... a later one accumulates; the last keeps no ctx and leaves the tile sums
    ws, nbytes = _op(lib, 0, q=fd.data_ptr() + 4 * (2 * C + 1), out=None, out2=total, accumulate=1, last=1, **common)
    _check("  ctx_all (accumulate)", total.permute(0, 3, 1, 2), ref * (gate[:, :1] + gate[:, 1:]).double(),
           t32 * gate[:, :1] + t32 * gate[:, 1:])
    tiles = ((H + 15) // 16) * ((W + 7) // 8)
    assert nbytes == B * tiles * C * 4
    sums = ws[:nbytes].view(torch.float32).view(B, tiles, C)
    _check("  tile sums", sums, _tile_sums(ref), _tile_sums(t32))


def test_focal_level_on_a_map_smaller_than_its_kernel():
    lib, C, k, (H, W), B = _hip.lib(), 1536, 9, (2, 3), 2           # the last stage of the fl4 case
    frow, w, ld = _level_inputs(C, H, W, k, 5)
    ref, t32 = _level_ref(frow, w, C, k, torch.float64), _level_ref(frow, w, C, k, torch.float32)
    fd, taps = frow.cuda(), w.reshape(C, k * k).t().contiguous().cuda()
    ctx, total = torch.empty(B, H, W, C, device="cuda"), torch.empty(B, H, W, C, device="cuda")
    ws, nbytes = _op(lib, 0, kind=3, x=fd.data_ptr() + 4 * C, weight=taps, q=fd.data_ptr() + 8 * C, out=ctx, out2=total,
                     batch=B, in_channels=C, height=H, width=W, out_channels=C, kernel_size=k, x_ld=ld, q_ld=ld, last=1)
    _check("level 2x3 k=9 ctx", ctx.permute(0, 3, 1, 2), ref, t32)
    _check("  tile sums", ws[:nbytes].view(torch.float32).view(B, 1, C), _tile_sums(ref), _tile_sums(t32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,hw", [(96, (20, 23)), (1536, (17, 9))])      # 6 and 4 tiles: the fixed-order sum is real
def test_modulator_finish_contract(C, hw, dtype):
    precision, rounding = ACT[dtype]
    lib, (H, W), B, k = _lib(dtype), hw, 2, 3
    frow, w, ld = _level_inputs(C, H, W, k, C + H)
    fd, taps = frow.cuda(), w.reshape(C, k * k).t().contiguous().cuda()
    total = torch.empty(B, H, W, C, device="cuda")
    ws = torch.empty((B * ((H + 15) // 16) * ((W + 7) // 8) * C + B * C) * 4, dtype=torch.uint8, device="cuda")
    _op(lib, precision, ws, kind=3, x=fd.data_ptr() + 4 * C, weight=taps, q=fd.data_ptr() + 8 * C, out=None, out2=total,
        batch=B, in_channels=C, height=H, width=W, out_channels=C, kernel_size=k, x_ld=ld, q_ld=ld, last=1)
    out = torch.empty(B, H, W, C, dtype=dtype, device="cuda")
    _, nbytes = _op(lib, precision, ws, kind=4, x=total, q=fd.data_ptr() + 4 * (2 * C + 1), out=out, batch=B, in_channels=C,
                    height=H, width=W, out_channels=C, q_ld=ld)
    assert nbytes == ws.numel()

    def statement(dt):
        ctx = _level_ref(frow, w, C, k, dt)
        g = frow[..., 2 * C:2 * C + 2].permute(0, 3, 1, 2).to(dt)
        return ctx * g[:, :1] + F.gelu(ctx.mean(2, keepdim=True).mean(3, keepdim=True)) * g[:, 1:]
    _check(f"finish C={C} {hw} {dtype}", out.permute(0, 3, 1, 2), statement(torch.float64), statement(torch.float32), rounding)


def _pack(lib, w, bias, scale, layout, precision, scale_bias=True):
    co, ci, k = w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)
    gamma = torch.ones(co) if scale is None else scale
    f32 = [t.float().contiguous().cuda() for t in (w, gamma, bias * gamma if scale_bias else bias, torch.zeros(co), torch.ones(co))]
    packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16, device="cuda")
    out_bias = torch.empty(co, device="cuda")
    _hip.launch("sdetr_backbone_pack", lib, packed.device, *[t.data_ptr() for t in f32], 0.0, co, ci, k, layout, precision,
                packed.data_ptr(), out_bias.data_ptr())
    return packed, out_bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,splits,out_f32", [(96, 1, 0), (192, 3, 0), (192, 2, 1)])
def test_h_with_the_product_epilogue_contract(C, splits, out_f32, dtype):
    precision, _ = ACT[dtype]
    lib, B, H, W = _lib(dtype), 2, 9, 15                            # 270 rows: two row tiles, the second ragged
    g = torch.Generator().manual_seed(C + splits)
    ld = (2 * C + 5 + 31) // 32 * 32
    frow = torch.randn(B, H, W, ld, generator=g)
    a = torch.randn(B, H, W, C, generator=g)
    w, bias = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5, 0.1 * torch.randn(C, generator=g)
    if precision == 1:
        a = a.to(dtype).float()
    ref = (F.linear(a.double(), w.double().view(C, C) * 0.2, bias.double())) * frow[..., :C].double()
    packed, pbias = _pack(lib, w, bias, torch.full((C,), 0.2), 0, precision, scale_bias=False)   # 1 / (L + 1) on the weight only
    out = torch.empty(B, H, W, C, dtype=torch.float32 if out_f32 else dtype, device="cuda")
    fd = frow.cuda()
    _, nbytes = _op(lib, precision, kind=2, x=a.to(dtype).cuda(), weight=packed, bias=pbias, q=fd, q_ld=ld, out=out, batch=B,
                    in_channels=C, height=H, width=W, out_channels=C, out_height=H, out_width=W, out_f32=out_f32, splits=splits)
    assert (nbytes > 0) == (splits > 1)
    d = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"h * q C={C} splits={splits} f32={out_f32} {dtype}: d / scale {d:.3g}")
    assert d <= (2e-6 if precision == 0 else 2e-2)


@pytest.mark.parametrize("dtype,out_f32,copy", [(torch.float32, 1, 0), (torch.bfloat16, 1, 1), (torch.bfloat16, 1, 0),
                                                (torch.float16, 1, 1), (torch.bfloat16, 0, 0), (torch.float16, 0, 0)])
@pytest.mark.parametrize("C", [32, 96, 384, 1536, 3072])     # 32: 8 lanes own a quad; 3072: all 12 quads of every lane
def test_layer_norm_scale_residual_contract(C, dtype, out_f32, copy):
    precision, rounding = ACT[dtype]
    lib = _lib(dtype)
    g = torch.Generator().manual_seed(C)
    x = 3 * torch.randn(2, 5, 7, C, generator=g) + 0.5
    res = torch.randn(2, 5, 7, C, generator=g) if out_f32 else None
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    scale = 0.1 + 0.2 * torch.rand(C, generator=g)                  # the layer scale, folded into the affine on the host

    def statement(dt):
        y = F.layer_norm(x.to(dt), (C,), (gamma * scale).to(dt), (beta * scale).to(dt), 1e-5)
        return y if res is None else res.to(dt) + y
    ref, t32 = statement(torch.float64), statement(torch.float32)
    out = torch.empty(2, 5, 7, C, dtype=torch.float32 if out_f32 else dtype, device="cuda")
    out2 = torch.empty(2, 5, 7, C, dtype=dtype, device="cuda") if copy else None
    _op(lib, precision, kind=5, x=x.cuda(), gamma=(gamma * scale).cuda(), beta=(beta * scale).cuda(),
        residual=None if res is None else res.cuda(), out=out, out2=out2, batch=2, in_channels=C, height=5, width=7,
        out_channels=C, out_f32=out_f32)
    _check(f"ln C={C} {dtype} f32={out_f32}", out, ref, t32, None if out_f32 else rounding)
    if copy:
        _check("  16-bit copy", out2, ref, t32, rounding)
        assert torch.equal(out2, out.to(dtype))                     # the same values, rounded once


@pytest.mark.parametrize("hw", [(5, 7), (9, 13)])                   # 35 pixels: one ragged block; 117: two
@pytest.mark.parametrize("C", [96, 352, 1536])
def test_layer_norm_to_nchw_contract(C, hw):
    lib, (H, W) = _hip.lib(), hw
    g = torch.Generator().manual_seed(C + H)
    x = 3 * torch.randn(2, H, W, C, generator=g) + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    statement = lambda dt: F.layer_norm(x.to(dt), (C,), gamma.to(dt), beta.to(dt), 1e-5).permute(0, 3, 1, 2)
    out = torch.empty(2, C, H, W, device="cuda")
    _op(lib, 0, kind=6, x=x.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), out=out, batch=2, in_channels=C, height=H, width=W,
        out_channels=C)
    _check(f"ln -> nchw C={C} {hw}", out, statement(torch.float64), statement(torch.float32))


EMBED_CASES = [  # (kernel, stride, padding, patch, in, out, (H, W), stem, splits)
    (7, 4, 2, 4, 3, 96, (29, 38), True, 1),          # the overlapped stem: 8 x 10 outputs, the floor size is 7 x 9
    (7, 4, 2, 4, 3, 96, (29, 38), True, 2),
    (3, 2, 1, 2, 96, 192, (13, 21), False, 1),       # the overlapped down-sampler: 7 x 11
    (3, 2, 1, 2, 96, 192, (13, 21), False, 4),
    (4, 4, 0, 4, 3, 96, (29, 38), True, 1),          # the patchify forms on sizes that need the padding
    (2, 2, 0, 2, 64, 160, (13, 21), False, 1),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EMBED_CASES)
def test_patch_embedding_contract(case, dtype):
    k, s, p, patch, ci, co, (H, W), stem, splits = case
    precision, _ = ACT[dtype]
    lib, B = _lib(dtype), 2
    g = torch.Generator().manual_seed(k * 100 + ci + co + splits)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    bias = 0.1 * torch.randn(co, generator=g)
    if precision == 1 and not stem:   # the 16-bit operand the kernel sees: compare against the same rounded values
        x = x.to(dtype).float()
    ho, wo = -(-H // patch), -(-W // patch)
    padded = F.pad(x.double(), (0, -W % patch, 0, -H % patch))      # the reference pads to a patch multiple first
    ref = F.conv2d(padded, w.double(), bias.double(), stride=s, padding=p)
    assert tuple(ref.shape[2:]) == (ho, wo)                         # ceil(H / patch): past the floor size but for 3 x 3 stride 2
    xd = x.cuda().contiguous() if stem else _rows(x).to(dtype).cuda()
    packed, pbias = _pack(lib, w, bias, None, 1 if stem else 0, precision)
    out = torch.empty(B, ho, wo, co, device="cuda")
    _, nbytes = _op(lib, precision, kind=0, x=xd, weight=packed, bias=pbias, out=out, batch=B, in_channels=ci, height=H,
                    width=W, out_channels=co, out_height=ho, out_width=wo, kernel_size=k, stride=s, padding=p,
                    x_nchw=int(stem), splits=splits)
    assert (nbytes > 0) == (splits > 1)
    d = (out.cpu().double().permute(0, 3, 1, 2) - ref).abs().max().item() / ref.abs().max().item()
    print(f"embed {case} {dtype}: d / scale {d:.3g}")
    assert d <= (2e-6 if precision == 0 else 2e-2)


# ---- the module against the imported reference --------------------------------------------------------------------

def _picked(t, ref):
    flat = t.reshape(-1).double().cpu()
    return flat if ref.size == flat.numel() else flat[FC.sub_index(flat.numel())]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_focalnet_fp32_matches_reference(gold, name):
    out = _run(_model(name), FC.canvas(name).cuda())
    assert list(out) == [f"layers.{i}.blocks" for i in FC.CASES[name][1]]
    for key, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous()
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        print(f"{name} fp32 {key}: d / bound {d / bound:.3f}")
        assert d <= bound, (key, d, bound)


@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("name", list(FC.CASES))
def test_focalnet_16bit_within_reference_autocast(gold, name, dtype, tag):
    out = _run(_model(name, dtype), FC.canvas(name).cuda())
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = 1.5 * gold[f"{name}.d{tag}_{key}"]
        print(f"{name} {tag} {key}: d / bound {d / bound:.3f}")
        assert d <= bound, (key, d, bound)


# ---- determinism, graphs, caches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_and_graph_replay_bit_identical(dtype):
    m, x = _model("fl4", dtype), FC.canvas("fl4").cuda()
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
    x = FC.canvas("hg").cuda()
    m = _model("hg")
    _run(m, x)                                     # packs the first weight set
    other = _model("hg", salt=99)
    m.load_state_dict(other.state_dict())
    a, b = _run(m, x), _run(other, x)
    for k in a:
        assert torch.equal(a[k], b[k])
    a = {k: v.clone() for k, v in a.items()}
    with torch.no_grad():                          # an in-place edit repacks too
        m.body.layers[0].blocks[0].gamma_1.mul_(2.0)
    c = _run(m, x)
    assert not torch.equal(c["layers.2.blocks"], a["layers.2.blocks"])


def test_16bit_parameters_compute_as_their_fp32_values():
    x = FC.canvas("srf").cuda()
    m16 = _model("srf").to(torch.bfloat16)
    m32 = _model("srf")
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    a, b = _run(m16, x), _run(m32, x)
    for k in a:
        assert torch.equal(a[k], b[k])


@pytest.mark.parametrize("name", ["srf", "hg"])
def test_composite_under_grad(name):
    m, x = _model(name), FC.canvas(name).cuda()
    out = m(x)                                     # grad enabled, parameters require grad
    with torch.no_grad():
        hip = m(x)
    for k in out:
        assert out[k].grad_fn is not None
        assert (hip[k] - out[k]).abs().max().item() <= 1e-4 * out[k].abs().max().item()


# ---- the detector from images --------------------------------------------------------------------------------------

def test_salience_detr_with_a_focalnet_backbone_equals_chain_by_hand():
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR, SalienceDETRHead
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    backbone = FocalNetBackbone(None, return_indices=(1, 2, 3), **FC.config("hg"))
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(50))
    sd = FC.syn.det_state_dict(det.state_dict(), salt=5)
    sd.update({"backbone." + k: v for k, v in FC.state(backbone.state_dict(), "hg").items()})
    det.load_state_dict(sd)
    det = det.eval().cuda()
    sizes = [(160, 224), (150, 200)]
    imgs = [FC.syn.det_rand(f"detector.img{i}", (3, h, w)).cuda() for i, (h, w) in enumerate(sizes)]
    got = det(imgs)
    with torch.no_grad():
        canvas, mask = batch_images(imgs)
        feats = det.backbone(canvas)
        want = SalienceDETRHead.forward(det, feats, mask, torch.tensor(sizes, device="cuda"),
                                        image_sizes=[list(s) for s in sizes], canvas=tuple(canvas.shape[-2:]))
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(a[k], b[k]), k
