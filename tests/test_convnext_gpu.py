"""GPU: the ConvNeXt backbone (csrc/convnext.hip): depthwise 7x7 + LayerNorm, LayerNorm, the patchify GEMMs with their
GELU and residual epilogues, and ``ConvNeXtBackbone``.

Each op against a float64 torch statement of its ABI contract; the module against the imported reference
(tests/golden/convnext_cases.npz, make_convnext_golden.py) in fp32 and under the reference's own autocast distance in
bf16 / fp16; run-to-run and graph-replay bit equality; the ``derived`` key after ``load_state_dict``; 16-bit parameters;
the composite under grad; the detector from images.

Whole network, worst d / bound per returned stage (first GPU run): not recorded yet, see DESIGN.md §4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_cases as CC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.backbone import batch_images
from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_cases.npz")
ACT = {torch.float32: (0, None), torch.bfloat16: (1, 2.0 ** -8), torch.float16: (1, 2.0 ** -11)}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, dtype=torch.float32, salt=None):
    m = ConvNeXtBackbone(None, return_indices=CC.CASES[name][2], block_setting=[CNBlockConfig(*r) for r in CC.setting(name)])
    m.load_state_dict(CC.state(m.state_dict(), name, salt))
    return m.eval().cuda().set_dtype(dtype)


def _canvas(name):
    return CC.canvas_and_mask(CC.images(name))[0].cuda()


def _run(m, x):
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    return out


def _op(lib, precision, ws_bytes=None, **kw):
    base = dict(kind=0, x=None, weight=None, bias=None, gamma=None, beta=None, residual=None, out=None, out_nchw=None,
                batch=1, in_channels=32, height=1, width=1, out_channels=32, kernel_size=1, stride=1, x_nchw=0, out_f32=0,
                splits=0, eps=1e-6)
    base.update({k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
    arr = (_hip.ConvnextOpStruct * 1)(_hip.ConvnextOpStruct(**base))
    nbytes = lib.sdetr_convnext_workspace_bytes(arr, 1, precision)
    assert nbytes >= 0, lib.sdetr_last_error().decode()
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.launch("sdetr_convnext_op_run", lib, ws.device, arr, precision, ws.data_ptr(), nbytes, what="convnext op")
    torch.cuda.synchronize()
    return nbytes


# ---- ops against their ABI contract --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hw,window", [((9, 13), None), ((20, 23), None), ((20, 23), (11, 17))])
@pytest.mark.parametrize("C", [96, 192, 1536])
def test_depthwise_layer_norm_contract(C, hw, window, dtype):
    precision, rounding = ACT[dtype]
    lib = _hip.lib(dtype if dtype == torch.float16 else None)
    g = torch.Generator().manual_seed(C + hw[0] + (7 if window else 0))
    B, (H, W) = 2, hw
    x = torch.randn(B, C, H, W, generator=g)
    if window is not None:                       # zero outside a sub-rectangle, as a padded canvas is
        x[:, :, window[0]:, :] = 0
        x[:, :, :, window[1]:] = 0
    w = torch.randn(C, 1, 7, 7, generator=g) / 7
    b, gamma, beta = (0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g))

    def ln(t, dt):
        y = F.conv2d(t.to(dt), w.to(dt), b.to(dt), padding=3, groups=C).permute(0, 2, 3, 1)
        return F.layer_norm(y, (C,), gamma.to(dt), beta.to(dt), 1e-6)
    ref, t32 = ln(x, torch.float64), ln(x, torch.float32).double()
    d_torch32 = (t32 - ref).abs().max().item()
    bound = max(2 * d_torch32, 1e-6 * ref.abs().max().item())
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    taps = w.reshape(C, 49).t().contiguous().cuda()
    out = torch.empty(B, H, W, C, dtype=dtype, device="cuda")
    _op(lib, precision, kind=2, x=xd, weight=taps, bias=b.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), out=out, batch=B,
        in_channels=C, height=H, width=W, out_channels=C, kernel_size=7)
    err = (out.cpu().double() - ref).abs()
    print(f"dw+ln C={C} {hw} {dtype}: d {err.max().item():.3g} d_torch32 {d_torch32:.3g} bound {bound:.3g}")
    if rounding is None:
        assert err.max().item() <= bound, (err.max().item(), bound)
    else:
        assert bool((err <= bound + rounding * ref.abs()).all()), (err - rounding * ref.abs()).max().item()


@pytest.mark.parametrize("dtype,out_f32", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 1), (torch.float16, 0)])
@pytest.mark.parametrize("C", [32, 96, 384, 1536, 3072])     # 32: 8 lanes own a quad; 3072: all 12 quads of every lane
def test_layer_norm_contract(C, dtype, out_f32):
    precision, rounding = ACT[dtype]
    lib = _hip.lib(dtype if dtype == torch.float16 else None)
    g = torch.Generator().manual_seed(C)
    x = 3 * torch.randn(2, 5, 7, C, generator=g) + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-6)
    d_torch32 = (F.layer_norm(x, (C,), gamma, beta, 1e-6).double() - ref).abs().max().item()
    out = torch.empty(2, 5, 7, C, dtype=torch.float32 if out_f32 else dtype, device="cuda")
    _op(lib, precision, kind=3, x=x.cuda(), gamma=gamma.cuda(), beta=beta.cuda(), out=out, batch=2, in_channels=C, height=5,
        width=7, out_channels=C, out_f32=out_f32)
    err = (out.cpu().double() - ref).abs()
    bound = max(2 * d_torch32, 1e-6 * ref.abs().max().item())
    if rounding is None or out_f32:
        assert err.max().item() <= bound, (err.max().item(), bound)
    else:
        assert bool((err <= bound + rounding * ref.abs()).all())


def _pack(lib, w, bias, scale, layout, precision):
    co, ci, k = w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)
    gamma = torch.ones(co) if scale is None else scale
    f32 = [t.float().contiguous().cuda() for t in (w, gamma, bias * gamma, torch.zeros(co), torch.ones(co))]
    packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16, device="cuda")
    out_bias = torch.empty(co, device="cuda")
    _hip.launch("sdetr_backbone_pack", lib, packed.device, *[t.data_ptr() for t in f32], 0.0, co, ci, k, layout, precision,
                packed.data_ptr(), out_bias.data_ptr())
    return packed, out_bias


GEMM_CASES = [  # (kind, kernel, in, out, residual, nchw copy, splits, stem)
    (1, 1, 96, 384, False, False, 1, False),        # Linear 1 + GELU
    (1, 1, 192, 200, False, False, 2, False),       # ragged output tile, split reduction
    (0, 1, 384, 96, True, True, 1, False),          # Linear 2 + residual + NCHW copy
    (0, 1, 384, 96, True, False, 3, False),
    (0, 2, 96, 192, False, False, 1, False),        # down-sampler
    (0, 2, 64, 160, False, True, 4, False),
    (0, 4, 3, 96, False, False, 1, True),           # stem on the NCHW canvas
    (0, 4, 3, 96, False, False, 2, True),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", GEMM_CASES)
def test_patchify_gemm_contract(case, dtype):
    kind, k, ci, co, with_res, with_nchw, splits, stem = case
    precision, _ = ACT[dtype]
    lib = _hip.lib(dtype if dtype == torch.float16 else None)
    g = torch.Generator().manual_seed(kind * 1000 + k * 100 + ci + co + splits)
    B, H, W = 2, 29, 38                                        # 29 is no multiple of 2 or 4: the last rows are dropped
    ho, wo = (H - k) // k + 1, (W - k) // k + 1
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    bias = 0.1 * torch.randn(co, generator=g)
    scale = 0.1 + 0.2 * torch.rand(co, generator=g) if with_res else None
    res = torch.randn(B, co, ho, wo, generator=g) if with_res else None
    if precision == 1 and not stem:   # the 16-bit operand the kernel sees: compare against the same rounded values
        x = x.to(dtype).float()
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=k)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.double()
    if kind == 1:
        ref = F.gelu(ref)
    xd = x.cuda().contiguous() if stem else x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()
    rd = None if res is None else res.permute(0, 2, 3, 1).contiguous().cuda()
    packed, pbias = _pack(lib, w, bias, scale, 1 if stem else 0, precision)
    out = torch.empty(B, ho, wo, co, dtype=dtype if kind == 1 else torch.float32, device="cuda")
    nchw = torch.empty(B, co, ho, wo, device="cuda") if with_nchw else None
    nbytes = _op(lib, precision, kind=kind, x=xd, weight=packed, bias=pbias, residual=rd, out=out, out_nchw=nchw, batch=B,
                 in_channels=ci, height=H, width=W, out_channels=co, kernel_size=k, stride=k, x_nchw=int(stem), splits=splits)
    assert (nbytes > 0) == (splits > 1)
    got = out.cpu().double().permute(0, 3, 1, 2)
    scale_ref = ref.abs().max().item()
    d = (got - ref).abs().max().item()
    print(f"gemm {case} {dtype}: d / scale {d / scale_ref:.3g}")
    assert d <= (2e-6 if precision == 0 else 2e-2) * scale_ref
    if nchw is not None:                                       # the stream is fp32 in every mode: the same values
        assert torch.equal(out.cpu().permute(0, 3, 1, 2), nchw.cpu())


# ---- the module against the imported reference --------------------------------------------------------------------

def _picked(t, ref):
    flat = t.reshape(-1).double().cpu()
    return flat if ref.size == flat.numel() else flat[CC.sub_index(flat.numel())]


@pytest.mark.parametrize("name", list(CC.CASES))
def test_convnext_fp32_matches_reference(gold, name):
    out = _run(_model(name), _canvas(name))
    assert list(out) == [f"features.{2 * i + 1}" for i in CC.CASES[name][2]]
    for key, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous()
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        print(f"{name} fp32 {key}: d / bound {d / bound:.3f}")
        assert d <= bound, (key, d, bound)


@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("name", list(CC.CASES))
def test_convnext_16bit_within_reference_autocast(gold, name, dtype, tag):
    out = _run(_model(name, dtype), _canvas(name))
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        print(f"{name} {tag} {key}: d / d{tag} {d / gold[f'{name}.d{tag}_{key}']:.3f}")
        assert d <= 1.5 * gold[f"{name}.d{tag}_{key}"], (key, d, gold[f"{name}.d{tag}_{key}"])


# ---- determinism, graphs, caches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_and_graph_replay_bit_identical(dtype):
    m, x = _model("cnl", dtype), _canvas("cnl")
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


def test_load_state_dict_repacks():
    x = _canvas("cnt4")
    m = _model("cnt4")
    _run(m, x)                                     # packs the first weight set
    other = _model("cnt4", salt=99)
    m.load_state_dict(other.state_dict())
    a, b = _run(m, x), _run(other, x)
    for k in a:
        assert torch.equal(a[k], b[k])
    with torch.no_grad():                          # an in-place edit repacks too
        m.features[1][0].layer_scale.mul_(2.0)
    c = _run(m, x)
    assert not torch.equal(c["features.1"], a["features.1"])


def test_16bit_parameters_compute_as_their_fp32_values():
    x = _canvas("cnt4")
    m16 = _model("cnt4").to(torch.bfloat16)
    m32 = _model("cnt4")
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    a, b = _run(m16, x), _run(m32, x)
    for k in a:
        assert torch.equal(a[k], b[k])


def test_composite_under_grad():
    m, x = _model("cnt4"), _canvas("cnt4")
    out = m(x)                                     # grad enabled, parameters require grad
    with torch.no_grad():
        hip = m(x)
    for k in out:
        assert out[k].grad_fn is not None
        assert (hip[k] - out[k]).abs().max().item() <= 1e-4 * out[k].abs().max().item()


# ---- the detector from images --------------------------------------------------------------------------------------

def test_salience_detr_with_a_convnext_backbone_equals_chain_by_hand():
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR, SalienceDETRHead
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    backbone = ConvNeXtBackbone(None, return_indices=(1, 2, 3), block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(50))
    sd = CC.syn.det_state_dict(det.state_dict(), salt=5)
    sd.update({"backbone." + k: v for k, v in CC.state(backbone.state_dict(), "cnt4").items()})
    det.load_state_dict(sd)
    det = det.eval().cuda()
    sizes = [(160, 224), (150, 200)]
    imgs = [CC.syn.det_rand(f"detector.img{i}", (3, h, w)).cuda() for i, (h, w) in enumerate(sizes)]
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
