"""GPU: the backbone (row N0, csrc/backbone.hip): folded-BN implicit-GEMM convolution, max pool, image batching and
``ResNetBackbone``.

Each kernel against a float64 torch statement of its ABI contract (kernel 1 / 3 / 7, stride 1 / 2, residual and ReLU on
and off, split and unsplit reduction, ragged tiles); the module against the imported reference
(tests/golden/backbone_cases.npz, make_backbone_golden.py) in fp32 and under the reference's own autocast distance in
bf16 / fp16; run-to-run and graph-replay bit equality; the ``derived`` key after ``load_state_dict``; 16-bit parameters;
the composite under grad."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backbone_cases as BC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd.backbone import FrozenBatchNorm2d, ResNetBackbone, batch_images

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, dtype=torch.float32, salt=None):
    arch, ret, _ = BC.CASES[name]
    m = ResNetBackbone(arch, return_indices=ret)
    sd = BC.state(m.state_dict(), name) if salt is None else BC.syn.det_state_dict(m.state_dict(), salt=salt)
    m.load_state_dict(sd)
    return m.eval().cuda().set_dtype(dtype)


def _canvas(name):
    canvas, _ = BC.canvas_and_mask(BC.images(name))
    return canvas.cuda()


def _run(m, x):
    with torch.no_grad():
        out = m(x)
    torch.cuda.synchronize()
    return out


# ---- kernels against their ABI contract ----------------------------------------------------------------------------

def _bn(co, seed):
    g = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(co)
    bn.weight.copy_(1 + 0.1 * torch.randn(co, generator=g))
    bn.bias.copy_(0.05 * torch.randn(co, generator=g))
    bn.running_mean.copy_(0.1 * torch.randn(co, generator=g))
    bn.running_var.copy_(0.5 + torch.rand(co, generator=g))
    return bn


def _pack(w, bn, layout, precision, lib):
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    f32 = [t.float().contiguous().cuda() for t in (w, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
    packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16, device="cuda")
    bias = torch.empty(co, device="cuda")
    _hip.check(lib.sdetr_backbone_pack(_hip.stream_ptr(), *[t.data_ptr() for t in f32], bn.eps, co, ci, k, layout,
                                       precision, packed.data_ptr(), bias.data_ptr()), "pack", lib)
    return packed, bias


def _folded64(w, bn):
    s = bn.weight.double() / (bn.running_var.double() + bn.eps).sqrt()
    return w.double() * s.view(-1, 1, 1, 1), bn.bias.double() - bn.running_mean.double() * s


CONV_CASES = [  # (kernel, stride, in, out, residual, relu, splits, nchw stem)
    (1, 1, 64, 96, False, True, 1, False),
    (1, 1, 256, 96, True, True, 3, False),
    (1, 2, 128, 64, False, False, 1, False),
    (3, 1, 64, 128, True, True, 1, False),
    (3, 1, 64, 160, False, True, 4, False),
    (3, 2, 96, 64, False, True, 2, False),
    (3, 2, 64, 64, True, False, 1, False),
    (7, 2, 3, 64, False, True, 1, True),
    (7, 2, 3, 64, False, True, 2, True),
]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_contract(case, precision):
    k, s, ci, co, with_res, relu, splits, nchw = case
    lib = _hip.lib()
    g = torch.Generator().manual_seed(k * 100 + s * 10 + ci + co + splits)
    B, H, W = 2, 29, 37
    p = (k - 1) // 2
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    bn = _bn(co, 7 + k)
    res = torch.randn(B, co, ho, wo, generator=g) if with_res else None
    act = torch.float32 if precision == 0 or nchw else torch.bfloat16
    if precision == 1:   # the 16-bit operands the kernel sees: compare against the same rounded values
        x = x.bfloat16().float()
        if res is not None:
            res = res.bfloat16().float()
    w64, b64 = _folded64(w, bn)
    ref = F.conv2d(x.double(), w64, b64, stride=s, padding=p)
    if res is not None:
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    xd = x.cuda().contiguous() if nchw else x.permute(0, 2, 3, 1).contiguous().to(act).cuda()
    out_act = torch.float32 if precision == 0 else torch.bfloat16
    rd = None if res is None else res.permute(0, 2, 3, 1).contiguous().to(out_act).cuda()
    packed, bias = _pack(w, bn, 1 if nchw else 0, precision, lib)
    out = torch.empty(B, ho, wo, co, dtype=out_act, device="cuda")
    out_nchw = torch.empty(B, co, ho, wo, device="cuda")
    op = (_hip.BackboneOpStruct * 1)(_hip.BackboneOpStruct(0, xd.data_ptr(), packed.data_ptr(), bias.data_ptr(), _hip.ptr(rd), out.data_ptr(),
                               out_nchw.data_ptr(), B, ci, H, W, co, k, s, p, int(relu), int(nchw), splits))
    steps = -(-ci * k * k // 32)                  # 32-deep reduction steps; the pieces are whole steps
    per = -(-steps // splits)
    assert lib.sdetr_backbone_conv_splits(op, precision) == -(-steps // per)
    nbytes = lib.sdetr_backbone_workspace_bytes(op, 1, precision)
    assert (nbytes > 0) == (splits > 1)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    _hip.check(lib.sdetr_backbone_conv(_hip.stream_ptr(), op, precision, ws.data_ptr(), nbytes), "conv", lib)
    torch.cuda.synchronize()
    got = out_nchw.cpu().double()
    scale = ref.abs().max().item()
    if precision == 0:
        assert (got - ref).abs().max().item() <= 2e-6 * scale
        assert torch.equal(out.cpu().permute(0, 3, 1, 2), out_nchw.cpu())
    else:   # one bf16 product of the rounded weight
        assert (got - ref).abs().max().item() <= 2e-2 * scale
        assert torch.equal(out.cpu().permute(0, 3, 1, 2), out_nchw.cpu().bfloat16())


def test_pack_is_the_exact_split_of_the_folded_weight():
    lib = _hip.lib()
    g = torch.Generator().manual_seed(3)
    w = torch.randn(80, 64, 3, 3, generator=g)
    bn = _bn(80, 5)
    packed, bias = _pack(w, bn, 0, 0, lib)
    planes = packed.cpu().view(3, 80, 576)
    as_f32 = lambda t: (t.to(torch.int32) << 16).view(torch.float32)
    total = as_f32(planes[0]).double() + as_f32(planes[1]).double() + as_f32(planes[2]).double()
    w64, b64 = _folded64(w, bn)
    order = w64.permute(0, 2, 3, 1).reshape(80, 576)   # k = (ky * 3 + kx) * C + c
    assert (total - order).abs().max().item() <= 5e-7 * order.abs().max().item()
    assert (bias.cpu().double() - b64).abs().max().item() <= 1e-6


def test_maxpool_exact():
    for precision, dt in ((0, torch.float32), (1, torch.bfloat16)):
        lib = _hip.lib()
        x = torch.randn(2, 33, 45, 64).to(dt).cuda()
        out = torch.empty(2, 17, 23, 64, dtype=dt, device="cuda")
        _hip.check(lib.sdetr_backbone_maxpool(_hip.stream_ptr(), x.data_ptr(), 2, 33, 45, 64, precision, out.data_ptr()),
                   "maxpool", lib)
        ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(dt)
        assert torch.equal(out, ref)


def test_batch_images_exact():
    imgs = BC.images("r50")
    canvas, mask = batch_images([i.cuda() for i in imgs])
    ref_c, ref_m = BC.canvas_and_mask(imgs)
    assert torch.equal(canvas.cpu(), ref_c) and torch.equal(mask.cpu(), ref_m)
    u8 = [(i * 255).round().to(torch.uint8) for i in imgs]
    canvas, mask = batch_images([i.cuda() for i in u8])
    ref_c, ref_m = BC.canvas_and_mask([i.float() / 255 for i in u8])
    assert torch.equal(canvas.cpu(), ref_c) and torch.equal(mask.cpu(), ref_m)


# ---- the module against the imported reference --------------------------------------------------------------------

def _picked(t, ref):
    flat = t.reshape(-1).double().cpu()
    return flat if ref.size == flat.numel() else flat[BC.sub_index(flat.numel())]


@pytest.mark.parametrize("name", list(BC.CASES))
def test_backbone_fp32_matches_reference(gold, name):
    out = _run(_model(name), _canvas(name))
    assert list(out) == [f"layer{i + 1}" for i in BC.CASES[name][1]]
    for key, t in out.items():
        assert t.dtype == torch.float32 and t.is_contiguous()
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        assert d <= bound, (key, d, bound)


@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
@pytest.mark.parametrize("name", ["r50", "r18", "r50_5"])
def test_backbone_16bit_within_reference_autocast(gold, name, dtype, tag):
    out = _run(_model(name, dtype), _canvas(name))
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        d = (_picked(t, ref) - torch.from_numpy(ref).double()).abs().max().item()
        assert d <= 1.5 * gold[f"{name}.d{tag}_{key}"], (key, d, gold[f"{name}.d{tag}_{key}"])


# ---- determinism, graphs, caches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_and_graph_replay_bit_identical(dtype):
    m, x = _model("r50", dtype), _canvas("r50")
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
    x = _canvas("r18")
    m = _model("r18")
    _run(m, x)                                     # packs the first weight set
    other = _model("r18", salt=99)
    m.load_state_dict(other.state_dict())
    a, b = _run(m, x), _run(other, x)
    for k in a:
        assert torch.equal(a[k], b[k])


def test_16bit_parameters_compute_as_their_fp32_values():
    x = _canvas("r18")
    m16 = _model("r18").to(torch.bfloat16)
    m32 = _model("r18")
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    a, b = _run(m16, x), _run(m32, x)
    for k in a:
        assert torch.equal(a[k], b[k])


def test_composite_under_grad():
    m, x = _model("r18"), _canvas("r18")
    out = m(x)                                     # grad enabled, parameters require grad
    assert all(t.requires_grad for t in out.values())
    ref = m.forward_torch(x)                       # (the library's conv algorithm choice may differ between calls)
    for k in out:
        assert out[k].grad_fn is not None
        assert (out[k] - ref[k]).abs().max().item() <= 1e-5 * ref[k].abs().max().item()
    with torch.no_grad():
        hip = m(x)
    for k in out:
        assert (hip[k] - out[k]).abs().max().item() <= 1e-4 * out[k].abs().max().item()


# ---- the detector from images --------------------------------------------------------------------------------------

def _detector():
    from salience_detr_amd.channel_mapper import ChannelMapper
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)
    det = SalienceDETR(ResNetBackbone("resnet50", return_indices=(1, 2, 3)), ChannelMapper([512, 1024, 2048], 256, 4),
                       PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(50))
    det.load_state_dict(BC.syn.det_state_dict(det.state_dict(), salt=5))
    return det.eval().cuda()


def test_salience_detr_from_images_equals_chain_by_hand():
    det = _detector()
    imgs = [BC.syn.det_rand(f"detector.img{i}", (3, h, w)).cuda() for i, (h, w) in enumerate([(160, 224), (150, 200)])]
    got = det(imgs)
    with torch.no_grad():
        canvas, mask = batch_images(imgs)
        feats = det.backbone(canvas)
        sizes = torch.tensor([[160, 224], [150, 200]], device="cuda")
        from salience_detr_amd.detector import SalienceDETRHead
        want = SalienceDETRHead.forward(det, feats, mask, sizes, image_sizes=[[160, 224], [150, 200]],
                                        canvas=tuple(canvas.shape[-2:]))
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(g[k], w[k]), k
    again = det(imgs)                              # run to run
    for g, w in zip(again, got):
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(g[k], w[k]), k


def test_batching_and_backbone_capture_and_replay():
    m = _model("r50", torch.bfloat16)
    imgs = BC.images("r50")
    imgs_d = [i.cuda() for i in imgs]

    def step():
        canvas, mask = batch_images(imgs_d)
        return [canvas, mask] + list(m(canvas).values())

    with torch.no_grad():
        eager = [t.clone() for t in step()]
        graph = graph_guard.new_graph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            step()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                out = step()
        torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, out):
        assert torch.equal(e, r)
