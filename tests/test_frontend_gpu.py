"""GPU: the detector's input stage (row N7, csrc/frontend.hip): ChannelMapper, level masks and sine positions.

Each kernel against a torch statement of its ABI contract (GroupNorm partials, split-K partial sums, ragged tiles), the
modules against the imported reference (tests/golden/frontend_cases.npz, make_frontend_golden.py), the ``derived`` key
after ``load_state_dict``, graph capture, and ``SalienceDETRHead`` against the same chain called module by module."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_cases as FC
from salience_detr_amd import _hip, graph_guard
from salience_detr_amd import synthetic as syn
from salience_detr_amd.channel_mapper import ChannelMapper
from salience_detr_amd.position_encoding import PositionEmbeddingSine, level_masks_and_positions

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _mapper(name, dtype=torch.float32, salt=None):
    cin, cout, num_outs, _, _ = FC.MAPPER_CASES[name]
    m = ChannelMapper(list(cin), cout, num_outs)
    sd = FC.mapper_state(m.state_dict(), name) if salt is None else syn.det_state_dict(m.state_dict(), salt=salt)
    m.load_state_dict(sd)
    return m.eval().cuda().set_dtype(dtype)


def _run_mapper(m, feats):
    with torch.no_grad():
        outs = m([f.cuda() for f in feats])
    torch.cuda.synchronize()
    return outs


# ---- kernels against their ABI contract ----------------------------------------------------------------------------

def _levels(specs):
    return (_hip.FrontendLevelStruct * len(specs))(*specs)


def _pack(w, precision, lib=None):
    """sdetr_frontend_pack_weight of an fp32 device weight -> int16 device tensor of its planes."""
    lib = lib or _hip.lib()
    w = w.contiguous()
    out = torch.empty(lib.sdetr_frontend_packed_bytes(w.numel(), precision) // 2, dtype=torch.int16, device=w.device)
    _hip.check(lib.sdetr_frontend_pack_weight(_hip.stream_ptr(), w.data_ptr(), w.numel(), precision, out.data_ptr()),
               "pack", lib)
    return out


@pytest.mark.parametrize("flavour", [torch.bfloat16, torch.float16])
def test_pack_weight_contract(flavour):
    """Precision 0: three planes whose fp32 sum is the weight exactly, each a truncated bf16; precision 1: one plane, the
    weight rounded to nearest in the library's 16-bit type."""
    lib = _hip.lib(flavour)
    w = torch.cat([syn.det_randn("fe.pack", (4099,)), torch.tensor([0.0, -0.0, 1e-30, -65504.0, 1 / 3, 3.0e38])]).cuda()
    n = w.numel()
    p3 = _pack(w, 0, lib).view(3, n)
    planes = [(p3[i].int() << 16).view(torch.float32) for i in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(planes[0] + planes[1] + planes[2], w)
    assert torch.equal(planes[0], ((w.view(torch.int32) >> 16) << 16).view(torch.float32))
    p1 = _pack(w[:n - 1], 1, lib)          # (3e38 left out: fp16 storage saturates where torch gives inf)
    assert torch.equal(p1.view(flavour), w[:n - 1].to(flavour))


@pytest.mark.parametrize("precision", [0, 1])
def test_conv_partials_and_split_k_contract(precision):
    """sdetr_frontend_conv: a ragged 1x1 level (P = 13 * 11, not a multiple of 4 or of the 128-pixel tile), a 1x1 level
    over two pixel tiles and a 3x3 stride-2 level split over K; raw outputs, (mean, M2) partials per (image, channel,
    pixel tile) and split partial sums against float64 torch."""
    B, co = 2, 160                           # two output-channel tiles, the second one partial
    shapes = [(64, 13, 11), (96, 12, 20), (256, 9, 14)]
    xs = [syn.det_randn(f"fe.k.x{i}", (B, c, h, w)).cuda() for i, (c, h, w) in enumerate(shapes)]
    ws = [(syn.det_randn(f"fe.k.w{i}", (co, c, k, k)) / (c * k * k) ** 0.5).cuda()
          for i, ((c, _, _), k) in enumerate(zip(shapes, (1, 1, 3)))]
    outs = [torch.full((B, co, h, w), float("nan"), device="cuda") for (_, h, w) in shapes[:2]]
    ones, zeros = torch.ones(co, device="cuda"), torch.zeros(co, device="cuda")
    wmat = [_pack(w.reshape(co, -1), precision) for w in ws]
    specs = [_hip.FrontendLevelStruct(xs[i].data_ptr(), wmat[i].data_ptr(), shapes[i][0], shapes[i][1], shapes[i][2],
                                      k, outs[i].data_ptr() if i < 2 else None, ones.data_ptr(), zeros.data_ptr())
             for i, k in enumerate((1, 1, 3))]
    arr = _levels(specs)
    lib = _hip.lib()
    nbytes = lib.sdetr_frontend_workspace_bytes(arr, 3, B, co)
    splits, offs = (ctypes.c_int * 3)(), (ctypes.c_int64 * 3)()
    _hip.check(lib.sdetr_frontend_conv_splits(arr, 3, B, co, splits, offs), "splits", lib)
    assert splits[0] == splits[1] == 1 and splits[2] > 1
    ws_buf = torch.full((nbytes // 4,), float("nan"), device="cuda")
    _hip.check(lib.sdetr_frontend_conv(_hip.stream_ptr(), arr, 3, B, co, precision, ws_buf.data_ptr(), nbytes), "conv", lib)
    torch.cuda.synchronize()
    tol = 2e-5 if precision == 0 else 1e-4
    for i in range(3):
        x64, w64 = xs[i].double().cpu(), ws[i].double().cpu()
        if precision == 1:
            x64, w64 = xs[i].bfloat16().double().cpu(), ws[i].bfloat16().double().cpu()
        want = F.conv2d(x64, w64, stride=1 if i < 2 else 2, padding=0 if i < 2 else 1)
        P = want.shape[2] * want.shape[3]
        base = offs[i] // 4
        if i < 2:
            got = outs[i].double().cpu()
            assert (got - want).abs().max().item() < tol
            tiles = (P + 127) // 128
            st = ws_buf[base:base + B * co * tiles * 2].view(B, co, tiles, 2).double().cpu()
            flat = got.reshape(B, co, P)
            for t in range(tiles):
                seg = flat[..., 128 * t:128 * (t + 1)]
                mean = seg.mean(-1)
                m2 = ((seg - mean[..., None]) ** 2).sum(-1)
                assert (st[..., t, 0] - mean).abs().max().item() < 1e-5
                assert ((st[..., t, 1] - m2).abs() / (1.0 + m2)).max().item() < 1e-5
        else:
            part = ws_buf[base:base + splits[2] * B * co * P].view(splits[2], B, co, P).double().cpu()
            got = part.sum(0).view_as(want)
            assert (got - want).abs().max().item() < tol


def test_groupnorm_contract_reduces_splits_in_place():
    """sdetr_frontend_groupnorm after the conv: GroupNorm with the affine over 1x1 levels in place and over the 3x3 level
    from its split partials, against F.group_norm of float64 convolutions."""
    B, co, groups = 2, 96, 32
    shapes = [(32, 7, 9), (64, 30, 45), (128, 11, 15)]
    ks = (1, 1, 3)
    xs = [syn.det_randn(f"fe.g.x{i}", (B, c, h, w)).cuda() for i, (c, h, w) in enumerate(shapes)]
    ws = [(syn.det_randn(f"fe.g.w{i}", (co, c, k, k)) / (c * k * k) ** 0.5 + 0.3).cuda()
          for i, ((c, _, _), k) in enumerate(zip(shapes, ks))]
    gam = [(1.0 + 0.1 * syn.det_randn(f"fe.g.g{i}", (co,))).cuda() for i in range(3)]
    bet = [(0.1 * syn.det_randn(f"fe.g.b{i}", (co,))).cuda() for i in range(3)]
    out_hw = [(h, w) if k == 1 else ((h - 1) // 2 + 1, (w - 1) // 2 + 1) for (_, h, w), k in zip(shapes, ks)]
    outs = [torch.empty(B, co, h, w, device="cuda") for h, w in out_hw]
    wmat = [_pack(w.reshape(co, -1), 0) for w in ws]
    arr = _levels([_hip.FrontendLevelStruct(xs[i].data_ptr(), wmat[i].data_ptr(), *shapes[i], ks[i], outs[i].data_ptr(),
                                            gam[i].data_ptr(), bet[i].data_ptr()) for i in range(3)])
    lib = _hip.lib()
    nbytes = lib.sdetr_frontend_workspace_bytes(arr, 3, B, co)
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    s = _hip.stream_ptr()
    _hip.check(lib.sdetr_frontend_conv(s, arr, 3, B, co, 0, buf.data_ptr(), nbytes), "conv", lib)
    _hip.check(lib.sdetr_frontend_groupnorm(s, arr, 3, B, co, groups, 1e-5, buf.data_ptr(), nbytes), "gn", lib)
    torch.cuda.synchronize()
    for i in range(3):
        y = F.conv2d(xs[i].double().cpu(), ws[i].double().cpu(), stride=1 if ks[i] == 1 else 2,
                     padding=0 if ks[i] == 1 else 1)
        want = F.group_norm(y, groups, gam[i].double().cpu(), bet[i].double().cpu(), 1e-5)
        assert outs[i].shape == want.shape
        assert (outs[i].double().cpu() - want).abs().max().item() < 2e-5


# ---- ChannelMapper against the reference ---------------------------------------------------------------------------

def _check_digest(gold, prefix, outs, tol):
    for l, o in enumerate(outs):
        o = o.cpu()
        if f"{prefix}.out{l}" in gold:
            assert (o - torch.from_numpy(gold[f"{prefix}.out{l}"])).abs().max().item() < tol, (prefix, l)
        assert (FC.sub_sample(o) - torch.from_numpy(gold[f"{prefix}.sub{l}"])).abs().max().item() < tol, (prefix, l)
        P = o.shape[2] * o.shape[3]
        assert (FC.channel_sums(o) - torch.from_numpy(gold[f"{prefix}.sum{l}"])).abs().max().item() < tol * P, (prefix, l)


@pytest.mark.parametrize("name", list(FC.MAPPER_CASES))
def test_mapper_fp32_matches_reference(gold, name):
    feats, _ = FC.mapper_inputs(name)
    m = _mapper(name)
    assert m.hip_form()
    outs = _run_mapper(m, feats)
    assert len(outs) == FC.MAPPER_CASES[name][2]
    _check_digest(gold, f"m.{name}", outs, 1e-4)


def test_mapper_takes_the_backbone_dict():
    """The backbone's dict goes in as the reference's does; the result equals the list form bit for bit."""
    feats, _ = FC.mapper_inputs("reduced")
    m = _mapper("reduced")
    a = _run_mapper(m, feats)
    with torch.no_grad():
        b = m({f"c{i}": f.cuda() for i, f in enumerate(feats)})
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ("reduced", "r50"))
@pytest.mark.parametrize("dtype,tag", [(torch.bfloat16, "bf16"), (torch.float16, "f16")])
def test_mapper_16bit_within_reference_autocast_distance(gold, name, dtype, tag):
    feats, _ = FC.mapper_inputs(name)
    outs = _run_mapper(_mapper(name, dtype), feats)
    for l, o in enumerate(outs):
        o = o.cpu()
        bound = 1.5 * float(gold[f"m.{name}.ac_{tag}{l}"])
        if f"m.{name}.out{l}" in gold:
            d = (o - torch.from_numpy(gold[f"m.{name}.out{l}"])).abs().max().item()
        else:
            d = (FC.sub_sample(o) - torch.from_numpy(gold[f"m.{name}.sub{l}"])).abs().max().item()
        assert o.dtype == torch.float32 and d <= bound, (l, d, bound)


def test_load_state_dict_equals_fresh_module():
    """The packed weight (a copy: three bf16 planes in fp32 mode, one 16-bit plane otherwise) is keyed on the parameters
    (derived.py): after load_state_dict of a second weight set the outputs equal a fresh module's bit for bit, in fp32
    and bf16; a stale packing would still compute with the first set."""
    feats, _ = FC.mapper_inputs("reduced")
    for dt in (torch.float32, torch.bfloat16):
        m = _mapper("reduced", dt, salt=3)
        _run_mapper(m, feats)
        fresh = _mapper("reduced", dt, salt=4)
        m.load_state_dict(fresh.state_dict())
        for a, b in zip(_run_mapper(m, feats), _run_mapper(fresh, feats)):
            assert torch.equal(a, b)


def test_write_through_data_then_invalidate_equals_fresh_module():
    from salience_detr_amd.derived import invalidate_caches
    feats, _ = FC.mapper_inputs("reduced")
    m = _mapper("reduced", salt=3)
    _run_mapper(m, feats)
    fresh = _mapper("reduced", salt=4)
    for p, q in zip(m.parameters(), fresh.parameters()):
        p.data.copy_(q.data)
    invalidate_caches(m)
    for a, b in zip(_run_mapper(m, feats), _run_mapper(fresh, feats)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_16bit_parameters_compute_as_their_fp32_values(pdt, cdt):
    """A mapper whose parameters are 16-bit (``.to(dtype)``, a 16-bit checkpoint) takes the HIP path on fp32 copies of
    them: bit-equal to an fp32 mapper holding the same values."""
    feats, _ = FC.mapper_inputs("reduced")
    m16 = _mapper("reduced").to(pdt).set_dtype(cdt)
    assert all(p.dtype == pdt for p in m16.parameters()) and m16.hip_form()
    cin, cout, num_outs, _, _ = FC.MAPPER_CASES["reduced"]
    m32 = ChannelMapper(list(cin), cout, num_outs)
    m32.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    m32 = m32.eval().cuda().set_dtype(cdt)
    for a, b in zip(_run_mapper(m16, feats), _run_mapper(m32, feats)):
        assert a.dtype == torch.float32 and torch.equal(a, b)


# ---- masks + positions ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FC.POSITION_CASES))
def test_masks_and_positions_match_reference(gold, name):
    kw, mask, shapes = FC.position_inputs(name)
    pe = PositionEmbeddingSine(**kw).cuda()
    masks, pos = level_masks_and_positions(mask.cuda(), shapes, pe)
    torch.cuda.synchronize()
    for l, (m, p) in enumerate(zip(masks, pos)):
        want_m = np.unpackbits(gold[f"p.{name}.mask{l}"])[:m.numel()].reshape(m.shape).astype(bool)
        assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), want_m), (name, l)
        p = p.cpu()
        if f"p.{name}.pos{l}" in gold:
            assert (p - torch.from_numpy(gold[f"p.{name}.pos{l}"])).abs().max().item() <= 2e-6, (name, l)
        else:
            assert (FC.sub_sample(p) - torch.from_numpy(gold[f"p.{name}.sub{l}"])).abs().max().item() <= 2e-6
            P = p.shape[2] * p.shape[3]
            assert (FC.channel_sums(p) - torch.from_numpy(gold[f"p.{name}.sum{l}"])).abs().max().item() <= 2e-6 * P
        if l == 0:   # the module's own forward on a level mask = the helper's map
            assert torch.equal(pe(masks[0]).cpu(), p)


# ---- graph capture -------------------------------------------------------------------------------------------------

def test_graph_capture_of_mapper_and_positions_replays_bit_for_bit():
    feats, mask = FC.mapper_inputs("r50")
    feats = [f.cuda() for f in feats]
    mask = mask.cuda()
    m = _mapper("r50")
    pe = PositionEmbeddingSine(128, 10000, True, offset=-0.5).cuda()

    def step():
        outs = m(feats)
        masks, pos = level_masks_and_positions(mask, [tuple(o.shape[-2:]) for o in outs], pe)
        return outs + masks + pos

    with torch.no_grad():
        eager = [t.clone() for t in step()]
        torch.cuda.synchronize()
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


# ---- the detector after its backbone -------------------------------------------------------------------------------

def test_salience_detr_head_equals_chain_by_hand():
    from salience_detr_amd.detector import SalienceDETRHead
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_transformer import build_salience_transformer
    feats, mask = FC.mapper_inputs("r50")
    tr = build_salience_transformer(topk_sa=32, two_stage_num_proposals=100)   # (a 160 x 224 canvas: few tokens)
    tr.load_state_dict(syn.det_state_dict(tr.state_dict()))
    head = SalienceDETRHead(_mapper("r50").cpu(), PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr,
                            PostProcess(50)).eval().cuda()
    sizes = torch.tensor(FC.MAPPER_CASES["r50"][4], device="cuda")
    f = [x.cuda() for x in feats]
    got = head(f, mask.cuda(), sizes)
    with torch.no_grad():
        nf = head.neck(f)
        lm = [FC.reference_level_mask(mask, o.shape[-2:]).cuda() for o in nf]
        pos = [head.position_embedding(x) for x in lm]
        cls, box = head.transformer(nf, lm, pos)[:2]
        want = head.postprocessor({"pred_logits": cls[-1], "pred_boxes": box[-1]}, sizes)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(g[k], w[k]), k
