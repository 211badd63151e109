"""Shared by tests/test_linear_x3_gpu.py and tests/test_zero_arena_gpu.py: the cases, runners and error bars of the
``X3Linear`` / ``x3_ffn`` parity checks (csrc/gemm_x3.hip against float64 autograd; the bar is a multiple of what torch's
own fp32 product loses on the same operands).  The float64 side of a case is computed once and shared."""
import functools

import torch

from salience_detr_amd import linear_x3 as X
from salience_detr_amd import synthetic as syn

DEV = "cuda"


def err(got, want64):
    return ((got.double().cpu() - want64).abs().max() / want64.abs().max()).item()


def ratio(got, ref, want64, factor=3.0, floor=3e-6):
    """Error of ``got`` as a fraction of its bar ``max(factor * err(ref), floor)`` (passes at <= 1)."""
    return err(got.detach(), want64.detach()) / max(factor * err(ref.detach(), want64.detach()), floor)


def assert_within_bar(got, ref, want, factor=3.0, floor=3e-6):
    """Every tensor of ``got`` within ``max(factor * (the fp32 reference's own error), floor)`` of float64; returns the
    worst error / bar."""
    worst = 0.0
    for g, r, w in zip(got, ref, want):
        assert err(g.detach(), w.detach()) <= max(factor * err(r.detach(), w.detach()), floor)
        worst = max(worst, ratio(g, r, w, factor, floor))
    return worst


# ---- X3Linear forward + backward ---------------------------------------------------------------------------------------
LINEAR_SHAPES = [((2, 1137, 256), 2048), ((3000, 2048), 256), ((2, 300, 256), 384)]


def force_every_product_through_x3(monkeypatch):
    for flag in ("X3_FORWARD", "X3_DX", "X3_DW"):   # all three products through the kernel under test
        monkeypatch.setattr(X, flag, True)
    monkeypatch.setattr(X, "X3_WIDE_OUT_ROWS", 1)
    monkeypatch.setattr(X, "X3_WIDE_FEATURES", 1)


@functools.lru_cache(maxsize=None)
def linear_operands(shape, N):
    K = shape[-1]
    lin = torch.nn.Linear(K, N)
    x = syn.det_randn(f"lx{N}", shape)
    gy = syn.det_randn(f"lg{N}", shape[:-1] + (N,))
    return lin.state_dict(), x, gy


@functools.lru_cache(maxsize=None)
def linear_float64(shape, N):
    """(y, dx, dw, db) of ``nn.Linear`` in float64 on the host."""
    sd, x, gy = linear_operands(shape, N)
    x64 = x.double().requires_grad_(True)
    l64 = torch.nn.Linear(shape[-1], N).double()
    l64.load_state_dict({k: v.double() for k, v in sd.items()})
    y = l64(x64)
    y.backward(gy.double())
    return y.detach(), x64.grad, l64.weight.grad, l64.bias.grad


def linear_device_run(shape, N, x3):
    """(y, dx, dw, db) of a fresh module on the device: ``X3Linear`` (``x3``) or torch's own fp32 ``nn.Linear``."""
    sd, x, gy = linear_operands(shape, N)
    xd = x.to(DEV).requires_grad_(True)
    ld = torch.nn.Linear(shape[-1], N).to(DEV)
    ld.load_state_dict(sd)
    if x3:
        assert X.use_x3_linear_(ld) == 1 and isinstance(ld, X.X3Linear)
        assert X.x3_linear_applies(xd, ld.weight, ld.bias)
    y = ld(xd)
    y.backward(gy.to(DEV))
    return y.detach(), xd.grad, ld.weight.grad, ld.bias.grad


# ---- x3_ffn --------------------------------------------------------------------------------------------------------------
FFN_CASES = [((2, 1137), True), ((2, 1137), False), ((2, 11363), None)]


def route_ffn(monkeypatch, wide):
    """wide = True / False forces every product through the x3 kernel / the library's GEMM; None = the shipped routing."""
    if wide is not None:
        monkeypatch.setattr(X, "X3_WIDE_OUT_ROWS", 1 if wide else 10 ** 9)
        monkeypatch.setattr(X, "X3_LONG_REDUCTION_ROWS", 1 if wide else 10 ** 9)


@functools.lru_cache(maxsize=None)
def ffn_operands(rows):
    l1, l2 = torch.nn.Linear(256, 2048), torch.nn.Linear(2048, 256)
    x = syn.det_randn("ffn_x", rows + (256,))
    gy = syn.det_randn("ffn_gy", rows + (256,))
    return l1.state_dict(), l2.state_dict(), x, gy


@functools.lru_cache(maxsize=None)
def ffn_float64(rows):
    """(y, dx, dw1, db1, dw2, db2) of ``linear2(relu(linear1(x)))`` in float64 on the host."""
    sd1, sd2, x, gy = ffn_operands(rows)
    x64 = x.double().requires_grad_(True)
    a64, b64 = torch.nn.Linear(256, 2048).double(), torch.nn.Linear(2048, 256).double()
    a64.load_state_dict({k: v.double() for k, v in sd1.items()})
    b64.load_state_dict({k: v.double() for k, v in sd2.items()})
    y64 = b64(torch.relu(a64(x64)))
    y64.backward(gy.double())
    return y64.detach(), x64.grad, a64.weight.grad, a64.bias.grad, b64.weight.grad, b64.bias.grad


def ffn_device_run(rows, fused):
    """The same six tensors from fresh ``X3Linear`` modules: ``x3_ffn`` (``fused``) or the two modules around ``relu``."""
    sd1, sd2, x, gy = ffn_operands(rows)
    m1, m2 = torch.nn.Linear(256, 2048).to(DEV), torch.nn.Linear(2048, 256).to(DEV)
    m1.load_state_dict(sd1)
    m2.load_state_dict(sd2)
    seq = torch.nn.Sequential(m1, m2)
    assert X.use_x3_linear_(seq) == 2
    xd = x.to(DEV).requires_grad_(True)
    if fused:
        assert X.x3_ffn_applies(xd, m1, m2)
        y = X.x3_ffn(xd, m1, m2)
    else:
        y = m2(torch.relu(m1(xd)))
    y.backward(gy.to(DEV))
    return y.detach(), xd.grad, m1.weight.grad, m1.bias.grad, m2.weight.grad, m2.bias.grad
