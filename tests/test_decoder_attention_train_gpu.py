"""The decoder's masked training attention (csrc/attention_train_masked.hip: key tiles, boolean mask) against float64
autograd of the textbook form, its fully-masked-row rule, the decoder layer's "hip" training form and graph replay.

The bar of the core comparisons is tests/test_attention_train_gpu.py's: the HIP result may be at most three times as far
from float64 as the fp32 torch composite on the device is (floor 3e-6), error = max abs difference over max abs value.
"""
import math

import pytest
import torch

from salience_detr_amd import attention_train as A
from salience_detr_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _err(got, want64):
    return ((got.double().cpu() - want64).abs().max() / max(1e-30, want64.abs().max().item())).item()


def _tile():
    from salience_detr_amd import _hip
    return _hip.lib().sdetr_attention_train_masked_tile_rows()


def _textbook(qk, v, H, mask=None, rows=None):
    """softmax(q k^T / sqrt(d) with masked_fill(-inf)) v, heads concatenated; ``rows``: only these query rows."""
    B, N, E = v.shape
    hd = E // H
    q = qk[..., :E].view(B, N, H, hd).transpose(1, 2)
    k = qk[..., E:].view(B, N, H, hd).transpose(1, 2)
    vv = v.view(B, N, H, hd).transpose(1, 2)
    if rows is not None:
        q = q[:, :, rows]
        mask = None if mask is None else mask[rows]
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    return (s.softmax(-1) @ vv).transpose(1, 2).reshape(B, q.shape[2], E)


def _random_mask(name, N):
    m = syn.det_rand(name, (N, N)) < 0.5
    m[torch.arange(N), torch.arange(N)] = False          # the diagonal is allowed: no fully masked row
    return m


def _late_start_mask(N, T):
    """More than one key tile.  Rows [0, 20): only keys of the LAST tile (every earlier tile is masked: m is still -inf
    when the first allowed key arrives).  Rows [N/2, N/2 + 20): only keys of the FIRST tile.  The last 10 rows: only keys
    j = 3 (mod 8), i.e. one lane of the row's eight ever sees a key.  Every other row sees everything."""
    assert N > T
    last = ((N - 1) // T) * T
    m = torch.zeros(N, N, dtype=torch.bool)
    m[:20, :last] = True
    m[N // 2:N // 2 + 20, T:] = True
    m[N - 10:, :] = True
    m[N - 10:, 3::8] = False
    return m


_cdn = {}


def _cdn_mask():
    """The mask GenerateCDNQueries makes for 900 matching queries and two images with 2 and 1 targets: 50 groups of
    2 x 2 denoising queries -> 1100 rows."""
    if "mask" not in _cdn:
        from salience_detr_amd.denoising import GenerateCDNQueries
        gen = GenerateCDNQueries(num_queries=900, num_classes=7, label_embed_dim=256, denoising_nums=100).to(DEV)
        labels = [torch.tensor([1, 4], device=DEV), torch.tensor([2], device=DEV)]
        boxes = [torch.tensor([[0.4, 0.5, 0.2, 0.3], [0.6, 0.3, 0.1, 0.2]], device=DEV),
                 torch.tensor([[0.5, 0.5, 0.4, 0.4]], device=DEV)]
        with torch.no_grad():
            _cdn["mask"] = gen(labels, boxes)[2]
    return _cdn["mask"]


def _mask(kind, N, T):
    if kind == "none":
        return None
    if kind == "cdn":
        m = _cdn_mask().cpu()
        assert m.dtype == torch.bool and tuple(m.shape) == (N, N)
        return m
    if kind == "random":
        return _random_mask(f"atm.mask{N}", N)
    return _late_start_mask(N, T)


def _run(qk, v, go, H, mask, dtype, device, native, rows=None):
    a = qk.to(device=device, dtype=dtype).requires_grad_(True)
    b = v.to(device=device, dtype=dtype).requires_grad_(True)
    mk = None if mask is None else mask.to(device)
    g = go.to(device=device, dtype=dtype)
    if native:
        o = A.attention_qk_v_masked(a, b, H, mk)
        o.backward(g)
        if rows is not None:
            o = o[:, rows]
    else:
        o = _textbook(a, b, H, mk, rows)
        o.backward(g if rows is None else g[:, rows])
    return o.detach(), a.grad, b.grad


# N: a number, or a function of the tile T.  Masks: each where it is defined (cdn: the 1100 rows the module makes for 900
# queries; late: more than one tile).
_SHAPES = [(1, "1", 1), (3, "5", 2), (1, "65", 4), (2, "T", 8), (1, "T+1", 8), (1, "2T+1", 2), (2, "1100", 8)]
_CASES = [(B, n, H, kind) for B, n, H in _SHAPES for kind in ("none", "random", "late", "cdn")
          if (kind != "cdn" or n == "1100") and (kind != "late" or n in ("T+1", "2T+1", "1100"))]


@pytest.mark.parametrize("B,n,H,kind", _CASES)
def test_masked_core_forward_backward_match_float64(B, n, H, kind):
    T = _tile()
    N = {"T": T, "T+1": T + 1, "2T+1": 2 * T + 1}.get(n) or int(n)
    E = 32 * H
    qk = syn.det_randn(f"atm.qk{N}{H}", (B, N, 2 * E)) * 1.5
    v = syn.det_randn(f"atm.v{N}{H}", (B, N, E))
    go = syn.det_randn(f"atm.g{N}{H}", (B, N, E))
    mask = _mask(kind, N, T)
    if mask is not None:
        assert not mask.all(1).any()                     # no fully masked row in this test
    want = _run(qk, v, go, H, mask, torch.float64, "cpu", False)
    assert all(torch.isfinite(w).all() for w in want)    # the float64 reference is NaN-free under this mask
    ref = _run(qk, v, go, H, mask, torch.float32, DEV, False)
    assert A.applies_masked(qk.to(DEV), v.to(DEV), H, None if mask is None else mask.to(DEV))
    got = _run(qk, v, go, H, mask, torch.float32, DEV, True)
    for name, g, f, w in zip(("out", "grad_qk", "grad_v"), got, ref, want):
        e_hip, e_ref = _err(g, w), _err(f, w)
        print(f"{name}: hip {e_hip:.3g} torch fp32 {e_ref:.3g}")
        assert torch.isfinite(g).all()
        assert e_hip <= max(3.0 * e_ref, 3e-6), name


def test_fully_masked_rows_give_zero_rows_and_no_gradient():
    """Rows 3 and 17 may attend to nothing (NaN in torch): output rows exactly 0, every result finite, and every other
    number equal to the float64 reference computed WITHOUT those two query rows."""
    B, N, H = 2, 40, 4
    E = 32 * H
    qk = syn.det_randn("atm.full.qk", (B, N, 2 * E)) * 1.5
    v = syn.det_randn("atm.full.v", (B, N, E))
    go = syn.det_randn("atm.full.g", (B, N, E))
    mask = _random_mask("atm.full.mask", N)
    mask[3] = True
    mask[17] = True
    keep = torch.tensor([i for i in range(N) if i not in (3, 17)])
    want = _run(qk, v, go, H, mask, torch.float64, "cpu", False, rows=keep)
    assert all(torch.isfinite(w).all() for w in want)
    ref = _run(qk, v, go, H, mask, torch.float32, DEV, False, rows=keep.to(DEV))
    a = qk.to(DEV).requires_grad_(True)
    b = v.to(DEV).requires_grad_(True)
    out = A.attention_qk_v_masked(a, b, H, mask.to(DEV))
    out.backward(go.to(DEV))
    out = out.detach()
    assert torch.isfinite(out).all() and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert (out[:, [3, 17]] == 0).all()
    assert (a.grad[:, [3, 17], :E] == 0).all()           # the q half of the fully masked rows
    got = (out[:, keep.to(DEV)], a.grad, b.grad)
    for name, g, f, w in zip(("out", "grad_qk", "grad_v"), got, ref, want):
        e_hip, e_ref = _err(g, w), _err(f, w)
        print(f"{name}: hip {e_hip:.3g} torch fp32 {e_ref:.3g}")
        assert e_hip <= max(3.0 * e_ref, 3e-6), name


def test_masked_core_saturated_logits_and_support():
    """Logits of +-80 under the random mask stay finite; what the kernel does not take is refused by `applies_masked`."""
    B, N, H = 1, 40, 8
    E = 32 * H
    qk = syn.det_randn("atm.big", (B, N, 2 * E)).to(DEV) * 9
    v = syn.det_randn("atm.bigv", (B, N, E)).to(DEV)
    mask = _random_mask("atm.big.mask", N)
    a, b = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o = A.attention_qk_v_masked(a, b, H, mask.to(DEV))
    o.sum().backward()
    assert torch.isfinite(o).all() and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    want = _textbook(qk.double().cpu(), v.double().cpu(), H, mask)
    assert torch.isfinite(want).all()
    assert _err(o, want) < 1e-5
    m = mask.to(DEV)
    assert A.applies_masked(qk, v, H, m) and A.applies_masked(qk, v, H, None)
    assert A.applies_masked(torch.zeros(1, 1500, 512, device=DEV), torch.zeros(1, 1500, 256, device=DEV), 8)   # no row limit
    assert not A.applies_masked(qk.bfloat16(), v.bfloat16(), H, m)
    assert not A.applies_masked(qk, v, H, m.float())                                       # additive mask
    assert not A.applies_masked(qk, v, H, m[None].expand(B * H, N, N))                     # per-head mask
    assert not A.applies_masked(qk, v, H, m[:, :-1])
    assert not A.applies_masked(qk, v, H, mask)                                            # mask on the CPU
    assert not A.applies_masked(qk.cpu(), v.cpu(), H, None)
    assert not A.applies_masked(torch.zeros(1, 10, 128, device=DEV), torch.zeros(1, 10, 64, device=DEV), 4)   # 16-channel heads
    # a non-contiguous mask is made contiguous once
    o2 = A.attention_qk_v_masked(qk, v, H, m.t().contiguous().t())
    assert torch.equal(o2, o.detach())


def _layer(dropout):
    from salience_detr_amd.salience_decoder import SalienceTransformerDecoder, SalienceTransformerDecoderLayer
    layer = SalienceTransformerDecoderLayer(embed_dim=256, d_ffn=64, n_heads=8, dropout=dropout, n_levels=1, n_points=1)
    dec = SalienceTransformerDecoder(layer, 1, 3).to(DEV).train()
    dec.set_train_form("hip")
    layer = dec.layers[0]
    with torch.no_grad():   # (the module's bias starts at zero: give every compared gradient a non-trivial operand)
        layer.self_attn.in_proj_bias.copy_(syn.det_randn("atm.layer.bias", (768,)).to(DEV) * 0.1)
    return layer


def _spy(monkeypatch):
    calls = []
    real = A.attention_qk_v_masked

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(A, "attention_qk_v_masked", spy)
    return calls


def test_decoder_layer_hip_form_equals_multihead_attention_module(monkeypatch):
    """The layer's "hip" training form (two in-projection GEMMs + the masked core + out-projection) against the same
    layer's nn.MultiheadAttention call under the boolean mask: output, parameter and input gradients."""
    B, N = 2, 130
    layer = _layer(0.0)
    assert layer.train_form == "hip" and layer.training
    calls = _spy(monkeypatch)
    mha = layer.self_attn
    mask = _random_mask("atm.layer.mask", N).to(DEV)
    w = syn.det_randn("atm.layer.w", (B, N, 256)).to(DEV)

    def run(hip):
        layer.zero_grad()
        q = syn.det_randn("atm.layer.q", (B, N, 256)).to(DEV).requires_grad_(True)
        pos = syn.det_randn("atm.layer.pos", (B, N, 256)).to(DEV).requires_grad_(True)
        out = layer._self_attention_train(q, pos, mask) if hip else layer._self_attention(q + pos, q, mask)
        (out * w).sum().backward()
        return (out.detach(), mha.in_proj_weight.grad.clone(), mha.in_proj_bias.grad.clone(),
                mha.out_proj.weight.grad.clone(), q.grad, pos.grad)

    got = run(True)
    assert len(calls) == 1
    want = run(False)
    assert len(calls) == 1
    for g, r in zip(got, want):
        assert (g - r).abs().max() <= 2e-5 * max(1.0, r.abs().max().item())


def test_decoder_layer_with_attention_dropout_takes_the_torch_path(monkeypatch):
    B, N = 1, 130
    layer = _layer(0.1)
    assert layer.train_form == "hip" and layer.training and layer.self_attn.dropout > 0
    calls = _spy(monkeypatch)
    mask = _random_mask("atm.layer.mask", N).to(DEV)
    q = syn.det_randn("atm.layer.q", (B, N, 256)).to(DEV).requires_grad_(True)
    pos = syn.det_randn("atm.layer.pos", (B, N, 256)).to(DEV)
    out = layer._self_attention_train(q, pos, mask)
    out.sum().backward()
    assert not calls and torch.isfinite(out).all() and torch.isfinite(q.grad).all()
    layer.eval()                                         # dropout inactive: the kernel serves the call
    layer._self_attention_train(q, pos, mask)
    assert len(calls) == 1
    layer.train()
    layer.train_form = "torch"                           # the default form never calls it
    layer.self_attn.dropout = 0.0
    layer._self_attention_train(q, pos, mask)
    assert len(calls) == 1


def test_masked_core_replays_in_a_captured_graph():
    """Forward + backward captured once on one stream, replayed twice with new contents in the static inputs: results
    bit-identical to eager calls, and output buffers filled with NaN before a replay come back NaN-free (every element
    of out, grad_qk and grad_v is written by the three launches)."""
    T = _tile()
    B, N, H = 2, T + 1, 8
    E = 32 * H
    mask = _random_mask("atm.graph.mask", N).to(DEV)
    inputs = [(syn.det_randn(f"atm.graph.qk{i}", (B, N, 2 * E)).to(DEV) * 1.5, syn.det_randn(f"atm.graph.v{i}", (B, N, E)).to(DEV),
               syn.det_randn(f"atm.graph.g{i}", (B, N, E)).to(DEV)) for i in range(3)]

    def eager(qk, v, go):
        a, b = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
        o = A.attention_qk_v_masked(a, b, H, mask)
        o.backward(go)
        return o.detach(), a.grad, b.grad

    want = [eager(*t) for t in inputs]                   # (also the eager warm-up)
    s_qk, s_v, s_go = (t.clone() for t in inputs[0])
    s_qk.requires_grad_(True)
    s_v.requires_grad_(True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            s_out = A.attention_qk_v_masked(s_qk, s_v, H, mask)
            s_gqk, s_gv = torch.autograd.grad(s_out, (s_qk, s_v), s_go)
    torch.cuda.current_stream().wait_stream(stream)
    for i in (1, 2):
        with torch.no_grad():
            s_qk.copy_(inputs[i][0])
            s_v.copy_(inputs[i][1])
            s_go.copy_(inputs[i][2])
            for t in (s_out, s_gqk, s_gv):
                t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip((s_out, s_gqk, s_gv), want[i]):
            assert not torch.isnan(g).any()
            assert torch.equal(g.detach(), w)
