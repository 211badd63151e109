"""Shared by tests/test_layer_norm_train_gpu.py and tests/test_zero_arena_gpu.py: operands, runner and error bar of the
``add_layer_norm`` parity check (csrc/layer_norm_train.hip against float64 autograd; the bar is a multiple of what torch's
own fp32 LayerNorm loses on the same operands)."""
import torch

from salience_detr_amd import layer_norm_train as L
from salience_detr_amd import synthetic as syn

DEV = "cuda"
FACTOR, FLOOR = 3.0, 2e-6


def err(got, want64):
    return ((got.double().cpu() - want64).abs().max() / max(1e-30, want64.abs().max().item())).item()


def operands(shape, with_residual):
    C = shape[-1]
    x = syn.det_randn(f"ln.x{shape}", shape) * 2 + 0.5
    r = syn.det_randn(f"ln.r{shape}", shape) if with_residual else None
    gy = syn.det_randn(f"ln.g{shape}", shape)
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(syn.det_randn(f"ln.w{C}", (C,)) * 0.3 + 1)
        norm.bias.copy_(syn.det_randn(f"ln.b{C}", (C,)))
    return x, r, gy, norm


def run(ops, dtype, device, fused):
    """(y, dx, dresidual | None, dweight, dbias) of a fresh LayerNorm: ``add_layer_norm`` (``fused``) or torch's own ops."""
    x, r, gy, norm = ops
    n = torch.nn.LayerNorm(x.shape[-1]).to(device=device, dtype=dtype)
    n.load_state_dict({k: v.to(dtype) for k, v in norm.state_dict().items()})
    xx = x.to(device=device, dtype=dtype).requires_grad_(True)
    rr = None if r is None else r.to(device=device, dtype=dtype).requires_grad_(True)
    if fused:
        assert L.applies(xx, n, rr)
    y = L.add_layer_norm(xx, n, rr) if fused else n(xx if rr is None else xx + rr)
    y.backward(gy.to(device=device, dtype=dtype))
    return y.detach(), xx.grad, None if rr is None else rr.grad, n.weight.grad, n.bias.grad


def assert_within_bar(got, ref, want):
    """Every tensor within ``max(3 * (torch's fp32 error), 2e-6)`` of float64; returns the worst error / bar."""
    worst = 0.0
    for g, f, w in zip(got, ref, want):
        if w is None:
            assert g is None
            continue
        bar = max(FACTOR * err(f, w), FLOOR)
        assert err(g, w) <= bar
        worst = max(worst, err(g, w) / bar)
    return worst
