"""GPU: the training step the way `bench.py` times it -- every zero-initialised fp32 buffer a slice of ONE arena cleared by
ONE fill kernel (salience_detr_amd/zero_arena.py).

The consumers of `zero_arena.zeros()` (linear_x3.py: split-reduction outputs and the `dw | db` pair; layer_norm_train.py:
`dwb`; ms_deform_attn.py: `grad_value` of both backward kernels) are otherwise tested with `torch.zeros` only, where every
buffer sits alone in an allocator block.  In the arena the buffers lie next to each other at arbitrary 256-byte offsets, stay
live until the next step and are made zero by one fill.  Every case here runs three ways -- arena off, served from a
`GuardedArena` (tests/zero_arena_cases.py) and the float64 / plain-C reference of the operator's own test -- and asserts

* the served result meets the bar the operator's own test states (the shared runners of tests/*_cases.py),
* no element outside the served slices (guard bands, alignment padding, tail) was written,
* where two arena-off runs are bit-equal (at two different placements), the served run is bit-equal too.

Then one mixed step (every buffer with live neighbours), a third step for the lifetime rule, the full 800x1333 step
eager and as a replayed hipGraph, the `bench.py` loss trajectory with and without the arena, and the two guards of
`ZeroArena` against reuse across a capture."""
import contextlib
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import layer_norm_cases as NC
import linear_x3_cases as LC
import msda_cases as MC
import train_step_compare as C
import zero_arena_cases as ZC

from salience_detr_amd import _hip, graph_guard
from salience_detr_amd import layer_norm_train as L
from salience_detr_amd import linear_x3 as X
from salience_detr_amd import ms_deform_attn as M
from salience_detr_amd import synthetic as syn
from salience_detr_amd import zero_arena as Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keep(out):
    """Copies of a run's tensors (a served gradient is a slice of the arena: the next step clears it)."""
    return tuple(None if t is None else t.detach().clone() for t in out)


def _bit_equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _off_again(fn):
    shift = torch.empty(1 << 20, device=DEV)     # (kept alive: this run's buffers land elsewhere than the last run's)
    out = _keep(fn())
    del shift
    return out


def _assert_bit_equal_if_deterministic(fn, off_a, off_b, got, what):
    """The determinism rule: two bit-equal arena-off runs make the operator deterministic, and ``got`` must then be
    bit-equal too.  Two runs of a sum of float atomics can agree by chance (three partial sums that happened to arrive in
    the same order), so before a difference counts as a failure the arena-off run is repeated up to four more times: one
    run that differs from the first shows that the operator is not deterministic, and the float64 bar is the check.  A
    deterministic operator whose served result differs fails as before.  Returns whether bit-equality was held."""
    if not _bit_equal(off_a, off_b):
        return False
    if _bit_equal(off_a, got):
        return True
    for _ in range(4):
        if not _bit_equal(off_a, _off_again(fn)):
            print("  %s: a later arena-off run differs from the first two -- not deterministic" % what)
            return False
    raise AssertionError("%s: arena-off runs are bit-equal, the arena-served result is not" % what)


def _three_ways(fn, what):
    """``fn()`` arena-off twice (the second run at another placement), then served from a fresh ``GuardedArena``.
    Asserts the clean guard bands and the determinism rule; returns (arena-off, served, arena)."""
    off_a = _keep(fn())
    off_b = _off_again(fn)
    served, arena = ZC.run_served(fn, DEV)
    served = _keep(served)
    torch.cuda.synchronize()
    dirty = ZC.dirty_guard_elements(arena)
    print("%s: %d slices served (%d floats), dirty guard elements %d, arena-off runs bit-equal: %s, served bit-equal to "
          "arena-off: %s" % (what, arena.fills_saved, arena.demand, dirty, _bit_equal(off_a, off_b), _bit_equal(off_a, served)))
    assert dirty == 0, what
    _assert_bit_equal_if_deterministic(fn, off_a, off_b, served, what)
    return off_a, served, arena


@pytest.fixture(params=["128x128 tiles", "256x128 tiles"])
def generation(request):
    with X.pinned_generation(1 if request.param.startswith("128") else 2):
        yield request.param


# ---- X3Linear: split-reduction outputs and the dw | db pair -----------------------------------------------------------
# rows / features that are no multiple of the 128 / 256 tiles; N * K no multiple of the arena's 64-float alignment for the
# first two (db starts at element N * K of its slice).  K % 8 != 0 leaves y with the library, N % 8 != 0 leaves dx there:
# dw | db goes through the kernel in every case
LINEAR_EDGE_SHAPES = [((1137, 36), 260), ((1001, 100), 132), ((1137, 256), 260), ((1001, 256), 384)]


@pytest.mark.parametrize("shape,N", LC.LINEAR_SHAPES + LINEAR_EDGE_SHAPES)
def test_x3_linear_served_from_the_arena(shape, N, monkeypatch, generation):
    LC.force_every_product_through_x3(monkeypatch)
    want = LC.linear_float64(shape, N)
    ref = LC.linear_device_run(shape, N, x3=False)
    off, served, arena = _three_ways(lambda: LC.linear_device_run(shape, N, x3=True), f"X3Linear {shape}->{N} {generation}")
    print("  worst error / bar: arena off %.3f, served %.3f" % (LC.assert_within_bar(off, ref, want),
                                                                LC.assert_within_bar(served, ref, want)))
    assert N * shape[-1] + N in [n for _, n in arena.extents], "dw | db was not one slice of the arena"


def test_every_split_reduction_of_x3_linear_is_among_the_cases(monkeypatch):
    LC.force_every_product_through_x3(monkeypatch)
    fwd, dx, dw = [], [], []
    for shape, N in LC.LINEAR_SHAPES + LINEAR_EDGE_SHAPES:
        K, T = shape[-1], int(np.prod(shape[:-1]))
        if K % 8 == 0 and X._x3_wide(T, N, K):
            fwd.append(X._reduction_splits(T, N, K))
        if N % 8 == 0 and X._x3_wide(T, K, N):
            dx.append(X._reduction_splits(T, K, N))
        dw.append(X._weight_grad_splits(T, N, K))
    assert max(fwd) > 1 and max(dx) > 1 and max(dw) > 1, (fwd, dx, dw)
    assert min(fwd) == 1 and min(dx) == 1, (fwd, dx)      # ... and the unsplit forms too


@pytest.mark.parametrize("rows,wide", LC.FFN_CASES)
def test_x3_ffn_served_from_the_arena(rows, wide, monkeypatch):
    LC.route_ffn(monkeypatch, wide)
    want = LC.ffn_float64(rows)
    plain = LC.ffn_device_run(rows, False)
    off, served, _ = _three_ways(lambda: LC.ffn_device_run(rows, True), f"x3_ffn {rows} wide={wide}")
    print("  worst error / bar: arena off %.3f, served %.3f" % (LC.assert_within_bar(off, plain, want),
                                                                LC.assert_within_bar(served, plain, want)))


# ---- add_layer_norm backward: dw | db ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [64, 128, 256, 512])
@pytest.mark.parametrize("rows", [(1,), (77,), (2, 11363)])
@pytest.mark.parametrize("with_residual", [True, False])
def test_add_layer_norm_served_from_the_arena(rows, C_, with_residual):
    assert _hip.lib().sdetr_layer_norm_train_supported(C_)
    ops = NC.operands(rows + (C_,), with_residual)
    want = NC.run(ops, torch.float64, "cpu", False)
    ref = NC.run(ops, torch.float32, DEV, False)
    off, served, arena = _three_ways(lambda: NC.run(ops, torch.float32, DEV, True),
                                     f"add_layer_norm {rows + (C_,)} residual={with_residual}")
    print("  worst error / bar: arena off %.3f, served %.3f" % (NC.assert_within_bar(off, ref, want),
                                                                NC.assert_within_bar(served, ref, want)))
    assert [n for _, n in arena.extents] == [2 * C_]


# ---- MSDA backward: grad_value of both kernels -------------------------------------------------------------------------
def _msda_three_ways(case, lds, what):
    """``lds``: True / False forces the LDS / the direct kernel, None leaves the library's dispatch.  Returns the kernel."""
    dev = case.on(DEV)
    kernels = []

    def run():
        with (MC.forced_backward_kernel(lds) if lds is not None else contextlib.nullcontext()):
            out = M.ms_deform_attn_backward(*dev, 64)
        kernels.append(M.last_backward_kernel())
        return tuple(out)

    off, served, arena = _three_ways(run, what)
    assert len(set(kernels)) == 1, kernels
    assert [n for _, n in arena.extents] == [case.value.numel()]
    print("  worst error / bar: arena off %.3f, served %.3f, kernel %d" % (
        case.assert_within_bar(*(t.cpu().numpy() for t in off)), case.assert_within_bar(*(t.cpu().numpy() for t in served)),
        kernels[0]))
    return kernels[0]


@pytest.mark.parametrize("B,Nq,levels,M_,D,P", MC.ORACLE_CASES)
def test_msda_backward_served_from_the_arena(B, Nq, levels, M_, D, P):
    """The cases of test_forward_backward_vs_c_oracle under the library's own dispatch: the direct kernel below
    ``lds_backward_min_queries`` queries, the LDS kernel from there."""
    case = MC.oracle_case(B, Nq, levels, M_, D, P, seed=1, spread=6.0, gout_name="gout")
    expect = M.KERNEL_BWD_DIRECT
    if Nq >= M.lds_backward_min_queries:
        assert _hip.lib().sdetr_msda_col2im_lds_supported(M_, D, len(levels), P, case.value.shape[1])
        expect = M.KERNEL_BWD_LDS
    assert _msda_three_ways(case, None, f"MSDA backward B={B} Nq={Nq} M={M_} D={D} L*P={len(levels) * P}") == expect


def test_msda_cases_reach_both_backward_kernels():
    assert {Nq >= M.lds_backward_min_queries for _, Nq, *_ in MC.ORACLE_CASES} == {True, False} and M.lds_backward


@pytest.mark.parametrize("B,Nq,levels,M_,spread", MC.LDS_CASES)
def test_msda_lds_backward_served_from_the_arena(B, Nq, levels, M_, spread):
    case = MC.oracle_case(B, Nq, levels, M_, 32, 4, seed=3, spread=spread, gout_name="gout_lds")
    assert _hip.lib().sdetr_msda_col2im_lds_supported(M_, 32, len(levels), 4, case.value.shape[1])
    assert _msda_three_ways(case, True, f"MSDA LDS backward B={B} Nq={Nq} M={M_} spread={spread}") == M.KERNEL_BWD_LDS


@pytest.mark.parametrize("lds", [False, True])
def test_msda_backward_with_locations_far_outside_the_maps(lds):
    """Sampling locations stretched ninefold around the centre, to about [-16, 17] (the maps are [0, 1]): most samples fall
    outside every level, the rest on its border, where a corner index that is not clamped would write in front of or behind
    grad_value."""
    case = MC.oracle_case(2, 333, MC.LEVELS_SMALL, 8, 32, 4, seed=6, spread=4.0, gout_name="gout_far",
                          loc_map=lambda loc: (loc - 0.5) * 9.0 + 0.5)
    assert case.loc.min() < -3.0 and case.loc.max() > 4.0
    assert _hip.lib().sdetr_msda_col2im_lds_supported(8, 32, 4, 4, case.value.shape[1])
    which = _msda_three_ways(case, lds, f"MSDA backward far outside, lds={lds}")
    assert which == (M.KERNEL_BWD_LDS if lds else M.KERNEL_BWD_DIRECT)


# ---- one mixed step: every zero buffer with live neighbours; a third step for the lifetime rule -------------------------
class _MixedStep:
    """Two X3Linear layers with an add_layer_norm between them (forward + backward), an MSDA backward through each kernel,
    and a second Linear chain of other sizes: under ONE ``arena.step()`` the split outputs, the ``dw | db`` pairs, the
    LayerNorm's ``dwb`` and both ``grad_value`` maps lie next to each other.  The modules persist across steps."""

    def __init__(self):
        def chain(tag, shape, hidden, out):
            l1, l2, norm = torch.nn.Linear(shape[-1], hidden), torch.nn.Linear(hidden, out), torch.nn.LayerNorm(hidden)
            with torch.no_grad():
                for name, q in (("w1", l1.weight), ("b1", l1.bias), ("w2", l2.weight), ("b2", l2.bias), ("g", norm.weight),
                                ("b", norm.bias)):
                    q.copy_(syn.det_randn(f"{tag}.{name}", tuple(q.shape)) * (0.3 if q.dim() == 1 else q.shape[1] ** -0.5))
                norm.weight.add_(1.0)
            return {"mods": (l1, l2, norm), "x": syn.det_randn(f"{tag}.x", shape),
                    "r": syn.det_randn(f"{tag}.r", shape[:-1] + (hidden,)), "gy": syn.det_randn(f"{tag}.gy", shape[:-1] + (out,))}

        self.host = [chain("mix.a", (2, 1137, 256), 512, 260), chain("mix.b", (1001, 100), 128, 132)]
        self.dev = []
        for c in self.host:
            mods = tuple(copy.deepcopy(m).to(DEV) for m in c["mods"])
            assert X.use_x3_linear_(torch.nn.Sequential(*mods)) == 2
            self.dev.append({"mods": mods, "x": c["x"].to(DEV).requires_grad_(True), "r": c["r"].to(DEV).requires_grad_(True),
                             "gy": c["gy"].to(DEV)})
        self.direct = MC.oracle_case(2, 333, MC.LEVELS_SMALL, 8, 32, 4, seed=1, spread=6.0, gout_name="gout")
        self.lds = MC.oracle_case(1, 700, MC.LEVELS_TILED, 3, 32, 4, seed=3, spread=4.0, gout_name="gout_lds")
        self.direct_dev, self.lds_dev = self.direct.on(DEV), self.lds.on(DEV)

    @staticmethod
    def _chain(c, fused):
        l1, l2, norm = c["mods"]
        h = l1(c["x"])
        if fused:
            assert L.applies(h, norm, c["r"])
        h = L.add_layer_norm(h, norm, c["r"]) if fused else norm(h + c["r"])
        y = l2(h)
        y.backward(c["gy"])
        return [y.detach(), c["x"].grad, c["r"].grad] + [p.grad for m in (l1, norm, l2) for p in m.parameters()]

    def float64(self):
        out = []
        for c in self.host:
            c64 = {"mods": tuple(copy.deepcopy(m).double() for m in c["mods"]), "x": c["x"].detach().double().requires_grad_(True),
                   "r": c["r"].detach().double().requires_grad_(True), "gy": c["gy"].double()}
            out += self._chain(c64, False)
        return out

    def step(self):
        """(the two chains' outputs and gradients, the two MSDA backwards' three gradients each); gradients start as None."""
        for c in self.dev:
            torch.nn.Sequential(*c["mods"]).zero_grad(set_to_none=True)
            c["x"].grad = c["r"].grad = None
        out = self._chain(self.dev[0], True)
        with MC.forced_backward_kernel(False):
            direct = M.ms_deform_attn_backward(*self.direct_dev, 64)
            assert M.last_backward_kernel() == M.KERNEL_BWD_DIRECT
        with MC.forced_backward_kernel(True):
            lds = M.ms_deform_attn_backward(*self.lds_dev, 64)
            assert M.last_backward_kernel() == M.KERNEL_BWD_LDS
        out += self._chain(self.dev[1], True)
        return tuple(out) + tuple(direct) + tuple(lds)

    def assert_within_bars(self, got, off, want):
        """The chains within the Linear bar (3 x what the arena-off step loses against float64, 3e-6 at least: arena on and
        off run the same kernels on the same operands), the MSDA gradients within 2e-4 of the C oracle."""
        n = len(want)
        worst = LC.assert_within_bar(got[:n], off[:n], want)
        return max(worst, self.direct.assert_within_bar(*(t.cpu().numpy() for t in got[n:n + 3])),
                   self.lds.assert_within_bar(*(t.cpu().numpy() for t in got[n + 3:n + 6])))


def test_mixed_step_with_live_neighbours_and_a_third_step(monkeypatch):
    LC.force_every_product_through_x3(monkeypatch)
    mixed = _MixedStep()
    want = mixed.float64()
    off = _keep(mixed.step())
    off_b = _off_again(mixed.step)
    second, arena = ZC.run_served(mixed.step, DEV)
    second = _keep(second)
    torch.cuda.synchronize()
    assert arena.fills_saved >= 8, arena.fills_saved       # 2 x (dw | db of both layers, dwb) + 2 grad_value maps
    assert ZC.dirty_guard_elements(arena) == 0
    print("mixed step: %d slices, worst error / bar: arena off %.3f, served %.3f" % (
        arena.fills_saved, mixed.assert_within_bars(off, off, want), mixed.assert_within_bars(second, off, want)))
    deterministic = _assert_bit_equal_if_deterministic(mixed.step, off, off_b, second, "mixed step")
    # ---- lifetime: the slices of the second step stay where they are until the third step's one fill; contents that
    # survived it would add to the third step's sums (an order-one error)
    slices = len(arena.extents)
    with arena.step():
        third = mixed.step()
    ZC.assert_fully_served(arena)
    third = _keep(third)
    torch.cuda.synchronize()
    assert len(arena.extents) == slices
    assert ZC.dirty_guard_elements(arena) == 0
    print("third step: worst error / bar %.3f, bit-equal to the second: %s" % (mixed.assert_within_bars(third, off, want),
                                                                              _bit_equal(second, third)))
    if deterministic:
        _assert_bit_equal_if_deterministic(mixed.step, off, off_b, third, "mixed step, third")


# ---- the full step, eager and replayed ---------------------------------------------------------------------------------
FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "hotpath_train_full.npz"))
CHECKED = tuple(FIXTURE["names"].tolist())


def _replay_bar(name):
    return 0.2 if ".linear1." in name else 1.5e-2      # tests/test_training_step_full_gpu.py, replay against eager


class _FullStep:
    """The set-up of tests/test_training_step_full_gpu.py (one 800x1333 image, the x3 Linear products), the step wrapped
    in ``arena.step()`` as bench.py's ``forward_backward`` wraps it."""

    def __init__(self):
        from salience_detr_amd.hot_path import build_hot_path
        from salience_detr_amd.linear_x3 import use_x3_linear_
        from salience_detr_amd.salience_filtering import replay_safe_mean
        m = build_hot_path(max_num_embedding=200)
        m.load_state_dict(syn.det_state_dict(m.state_dict()))
        self.sizes = [(800, 1333)]
        _, masks = syn.make_masks(self.sizes)
        self.canvas = syn.pad_to_32(*self.sizes[0])
        shapes = [tuple(x.shape[-2:]) for x in masks]
        feats = syn.make_feats(1, shapes, 256, seed=0)
        pos = [syn.sine_position_embedding(x, 128) for x in masks]
        self.m = m.to(DEV).train()
        use_x3_linear_(self.m)
        self.params = dict(self.m.named_parameters())
        self.f, self.k, self.p = ([t.to(DEV) for t in ts] for ts in (feats, masks, pos))
        self.w = None
        self.mean = replay_safe_mean

    def forward_backward(self, arena):
        self.m.zero_grad(set_to_none=True)
        with (arena.step() if arena is not None else contextlib.nullcontext()):
            memory, score_maps = self.m(self.f, self.k, self.p, image_sizes=self.sizes, canvas=self.canvas)
            if self.w is None:
                self.w = syn.det_randn("train_full.w", tuple(memory.shape)).to(DEV)
            loss = C.loss_fn(memory, score_maps, self.w, self.mean)
            loss.backward()
        return loss.detach()

    def grads(self):
        return {n: q.grad.detach().clone() for n, q in self.params.items() if q.grad is not None}

    def capture(self, arena):
        """As bench.py's ``capture``: one step on a side stream, then the capture into a graph whose handle is kept."""
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.forward_backward(arena)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = graph_guard.new_graph()
        with torch.cuda.graph(g):
            loss_static = self.forward_backward(arena)
        return g, loss_static


@pytest.fixture(scope="module")
def full_step():
    s = _FullStep()
    s.forward_backward(None)                  # (the first step also builds the derived operands)
    s.off_loss = s.forward_backward(None).item()
    s.off = s.grads()
    s.arena = ZC.GuardedArena(DEV)
    s.forward_backward(s.arena)               # sizing
    with C.record_top300(s.m) as (picked, lists):
        s.served_loss = s.forward_backward(s.arena).item()
    torch.cuda.synchronize()
    ZC.assert_fully_served(s.arena)
    s.picked, s.lists = picked, lists
    s.served = s.grads()
    s.served_dirty = ZC.dirty_guard_elements(s.arena)
    s.served_slices = s.arena.fills_saved
    print("full step: %d buffers served per step from %d floats" % (s.arena.fills_saved, s.arena.buf.numel()))
    yield s
    del s.m, s.params, s.arena


def test_served_full_step_matches_the_reference_fixture(full_step):
    s = full_step
    want = float(FIXTURE["loss"])
    assert abs(s.served_loss - want) < 2e-3 * max(1.0, abs(want)), (s.served_loss, want)
    assert len(s.picked) == 6 and len(s.lists) == 1
    for kk in range(6):
        assert set(FIXTURE[f"sel_tokens{kk}"][0].tolist()) == set(s.lists[0][0][s.picked[kk][0]].tolist()), kk
    worst = {}
    for n in CHECKED:
        v, off = C.compare(C.sub(s.served[n].cpu()), torch.from_numpy(FIXTURE["grad." + n]), n, float(FIXTURE["scale." + n]))
        worst[n] = v
        assert v < 1e-2 and off <= 20, (n, v, off)
    print("served eager step against the reference's own gradients: worst %.6f (%s)" % (max(worst.values()),
                                                                                        max(worst, key=worst.get)))


def test_served_full_step_matches_the_arena_off_step(full_step):
    s = full_step
    assert abs(s.served_loss - s.off_loss) < 1e-4 * max(1.0, abs(s.off_loss)), (s.served_loss, s.off_loss)
    assert set(s.served) == set(s.off) and len(s.off) >= 100, (len(s.served), len(s.off))
    worst = {}
    for n, ge in s.off.items():
        gs = s.served[n]
        assert torch.isfinite(gs).all(), n
        worst[n] = ((gs - ge).abs().max() / max(ge.abs().max().item(), 1e-6)).item()
    print("served against arena-off over all %d parameters: worst %.5f (%s)" % (len(worst), max(worst.values()),
                                                                                max(worst, key=worst.get)))
    bad = {n: round(v, 5) for n, v in worst.items() if v > _replay_bar(n)}
    assert not bad, bad
    assert s.served_dirty == 0


def test_replayed_full_step_with_the_arena(full_step):
    s = full_step
    g, loss_static = s.capture(s.arena)
    inspected = graph_guard.assert_replay_safe(g, "training step with the zero arena")
    ZC.assert_fully_served(s.arena)
    assert s.arena.captured and s.arena.fills_saved == s.served_slices
    ptr = s.arena.buf.data_ptr()
    captured = {n: s.params[n].grad for n in s.served}
    assert all(t is not None for t in captured.values())
    for _ in range(3):   # replays on a poisoned arena and poisoned gradients: what is there afterwards is the graph's work
        s.arena.buf.fill_(float("nan"))
        for t in captured.values():
            t.fill_(float("nan"))
        loss_static.fill_(float("nan"))
        g.replay()
    torch.cuda.synchronize()
    assert s.arena.buf.data_ptr() == ptr
    assert abs(loss_static.item() - s.served_loss) < 1e-4 * max(1.0, abs(s.served_loss)), (loss_static.item(), s.served_loss)
    worst = {}
    for n, ge in s.served.items():
        gc = captured[n]
        assert torch.isfinite(gc).all(), n
        worst[n] = ((gc - ge).abs().max() / max(ge.abs().max().item(), 1e-6)).item()
    print("replay against the served eager step over all %d parameters: worst %.5f (%s)" % (
        len(worst), max(worst.values()), max(worst, key=worst.get)))
    bad = {n: round(v, 5) for n, v in worst.items() if v > _replay_bar(n)}
    assert not bad, bad
    assert ZC.dirty_guard_elements(s.arena) == 0
    if inspected > 0:    # node handles available: the arena-off step as a graph holds one fill per buffer more
        g_off, _ = s.capture(None)
        off_nodes = len(graph_guard.node_types(g_off))
        print("captured training step: %d graph nodes with the arena, %d without" % (inspected, off_nodes))
        assert inspected < off_nodes, (inspected, off_nodes)
        del g_off
    else:
        print("captured training step: this torch exposes no graph handle, node counts not compared")


def _last_json(text):
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            return json.loads(line)
    raise AssertionError("no JSON line in:\n" + text[-2000:])


def test_bench_trajectory_with_and_without_the_arena():
    """`bench.py --mode train`: the loss three AdamW updates after the initial state is the same number with the arena
    (the default) and with `--no-zero-arena` (tests/test_rccl_path_gpu.py's pattern and bar)."""
    common = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--mode", "train", "--steps", "3", "--warmup", "1"]
    runs = []
    for extra in ([], ["--no-zero-arena"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ))
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(_last_json(r.stdout))
    on, off = runs
    print("bench.py losses: arena on %.6f, off %.6f; zero_arena %s; graph nodes %s / %s" % (
        on["loss"], off["loss"], on["config"]["zero_arena"], on["config"]["hipgraph_nodes"], off["config"]["hipgraph_nodes"]))
    assert on["config"]["zero_arena"]["buffers_served_per_step"] > 0
    assert off["config"]["zero_arena"] is None
    assert abs(on["loss"] - off["loss"]) <= 1e-4 * max(1.0, abs(on["loss"])), (on["loss"], off["loss"])


# ---- the guards of ZeroArena against reuse across a capture ------------------------------------------------------------
def _tiny_step(arena, out, sizes):
    """A few tiny fills: every requested buffer gets its index + 1 added and lands in ``out``."""
    with arena.step():
        at = 0
        for i, n in enumerate(sizes):
            t = Z.zeros(n, torch.float32, DEV)
            t.add_(float(i + 1))
            out[at:at + n].copy_(t)
            at += n


def _expected(sizes):
    return torch.cat([torch.full((n,), float(i + 1)) for i, n in enumerate(sizes)])


def _capture_tiny(arena, out, sizes):
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _tiny_step(arena, out, sizes)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = graph_guard.new_graph()
    with torch.cuda.graph(g):
        _tiny_step(arena, out, sizes)
    return g


def test_capture_without_a_sizing_step_raises():
    out = torch.zeros(400, device=DEV)
    arena = Z.ZeroArena(DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="sizing step before capturing"):
        with torch.cuda.graph(g):
            out.add_(1.0)                      # (one kernel node, so that the abandoned capture is not empty)
            _tiny_step(arena, out, (100, 7))
    torch.cuda.synchronize()
    assert arena.buf is None and not arena.captured
    # ... and a buffer that is too small for what the captured step asks
    _tiny_step(arena, out, (100,))
    assert arena.buf is not None
    ptr = arena.buf.data_ptr()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="sizing step before capturing"):
        with torch.cuda.graph(g):
            out.add_(1.0)
            _tiny_step(arena, out, (100, 300))
    torch.cuda.synchronize()
    assert arena.buf.data_ptr() == ptr and not arena.captured


def test_a_larger_step_after_capture_raises_and_keeps_the_buffer():
    sizes = (100, 7, 65)
    out = torch.zeros(sum(sizes) + 5000, device=DEV)
    arena = Z.ZeroArena(DEV)
    _tiny_step(arena, out, sizes)              # sizing
    g = _capture_tiny(arena, out, sizes)
    assert arena.captured
    ptr = arena.buf.data_ptr()
    with pytest.raises(RuntimeError, match="demand grew after capture"):
        _tiny_step(arena, out, sizes + (5000,))
    assert arena.buf.data_ptr() == ptr
    arena.buf.fill_(float("nan"))
    out.fill_(float("nan"))
    g.replay()                                 # the graph still owns the addresses it was captured with
    torch.cuda.synchronize()
    assert torch.equal(out[:sum(sizes)].cpu(), _expected(sizes))


def test_sizing_then_capture_then_replay_is_untouched():
    sizes = (100, 7, 65)
    out = torch.zeros(sum(sizes), device=DEV)
    arena = Z.ZeroArena(DEV)
    _tiny_step(arena, out, sizes)
    assert arena.fills_saved == 0
    g = _capture_tiny(arena, out, sizes)
    assert graph_guard.assert_replay_safe(g, "tiny arena steps") >= 0
    assert arena.captured and arena.fills_saved == len(sizes)
    ptr = arena.buf.data_ptr()
    for _ in range(3):
        arena.buf.fill_(float("nan"))
        out.fill_(float("nan"))
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _expected(sizes)) and arena.buf.data_ptr() == ptr
    _tiny_step(arena, out, sizes)              # an eager step of the same size goes on being served
    torch.cuda.synchronize()
    assert arena.fills_saved == len(sizes) and arena.buf.data_ptr() == ptr and torch.equal(out.cpu(), _expected(sizes))
