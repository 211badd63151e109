"""GPU: the optimizer step through its two kernels (csrc/optimizer.hip) -- the reference's float64 trajectories, run-to-run
and graph-replay bit-identity, torch's own device AdamW, the edge behaviours, the ``_version`` bump the ``derived()``
caches depend on, tensor layouts, the reducer's gradients, and four training steps of the detector, eager and as one graph.

The bound of a trajectory is max(4 * d_ref, k * ulp32(max|tensor|)) for tensors and max(4 * d_ref_norm, 2^-22) for the
norm; the tests print their worst error / bound ratios (none has been recorded from a device run yet)."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import optimizer_cases as OC
from salience_detr_amd import graph_guard
from salience_detr_amd.optimizer import ClippedAdamW

pytestmark = pytest.mark.gpu
_KERNEL_NODE = 0     # hipGraphNodeTypeKernel


@pytest.fixture(scope="module")
def fx():
    return OC.Fixture()


def _fixture_run(fx, steps=None, scheduler=True):
    params = fx.params("cuda")
    opt = ClippedAdamW(fx.groups(params), max_norm=fx.max_norm)
    advance = fx.schedulers(opt) if scheduler else (lambda k: None)
    out = []
    for k in range(fx.steps if steps is None else steps):
        for i, p in enumerate(params):
            p.grad = fx.gradient(k, i, "cuda")
        opt.step()
        advance(k)
        out.append(([tuple(t.detach().clone() for t in tr) for tr in OC.state_triples(opt, params)],
                    opt.last_grad_norm.clone()))
    return out


def test_trajectory_parity_with_the_float64_reference(fx):
    worst = []
    for k, (triples, norm) in enumerate(_fixture_run(fx)):
        fx.check_step(k, triples, float(norm), worst=worst)
    print("optimizer trajectory: worst error / bound per step (tensors, norm):", worst)


def test_two_runs_are_bit_identical(fx):
    a, b = _fixture_run(fx), _fixture_run(fx)
    for (ta, na), (tb, nb) in zip(a, b):
        assert torch.equal(na, nb)
        for x, y in zip(ta, tb):
            assert all(torch.equal(u, v) for u, v in zip(x, y))


def test_graph_replay_equals_eager_steps(fx):
    """K replays of a graph of ``step_captured()`` against K eager ``step()`` calls: new gradients and a new ``lr``
    between replays, bit-identical parameters, moments and norms; two kernel nodes, no memset node."""
    K = 4
    skip = fx.none_grad[1]          # static gradient buffers: every tensor has one at every step
    grad = lambda k, i: fx.gradient(k, i, "cuda") if i != skip or k != fx.none_grad[0] else torch.zeros(fx.shapes[i], device="cuda")
    eager_p = fx.params("cuda")
    eager = ClippedAdamW(fx.groups(eager_p), max_norm=fx.max_norm)
    norms = []
    for k in range(K):
        for i, p in enumerate(eager_p):
            p.grad = grad(k, i)
        for gi, g in enumerate(eager.param_groups):
            g["lr"] = float(fx.lrs[k][gi])
        eager.step()
        norms.append(eager.last_grad_norm.clone())

    params = fx.params("cuda")
    opt = ClippedAdamW(fx.groups(params), max_norm=fx.max_norm)
    for i, p in enumerate(params):
        p.grad = torch.zeros_like(p)                    # fixed addresses: the replays read these
    for gi, g in enumerate(opt.param_groups):
        g["lr"] = float(fx.lrs[0][gi])
    opt.prepare()
    torch.cuda.synchronize()
    graph = graph_guard.new_graph()
    with torch.cuda.graph(graph):
        opt.step_captured()
    types = graph_guard.node_types(graph)
    assert types, "no graph handle: the launch count and the memset check could not be made"
    assert graph_guard.assert_replay_safe(graph, "captured optimizer step") == 2
    assert types.count(_KERNEL_NODE) == 2 and len(types) == 2, types
    for k in range(K):
        for i, p in enumerate(params):
            p.grad.copy_(grad(k, i))
        versions = [p._version for p in params]
        graph.replay()
        assert torch.equal(opt.last_grad_norm, norms[k])
        for gi, g in enumerate(opt.param_groups):       # the scheduler's part: the next step's learning rates
            g["lr"] = float(fx.lrs[min(k + 1, K - 1)][gi])
        opt.after_replay()
        assert all(p._version > v for p, v in zip(params, versions))
    torch.cuda.synchronize()
    for a, b in zip(OC.state_triples(opt, params), OC.state_triples(eager, eager_p)):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert float(opt.state_dict()["state"][0]["step"]) == K


def test_against_torch_adamw_on_the_device(fx):
    """``clip_grad_norm_`` + ``torch.optim.AdamW(fused=False)`` on the device, held to the same float64 fixture: its own
    distance is the ``d_ref`` this class has to stay within four times of (or the rounding floor)."""
    params = fx.params("cuda")
    ref = torch.optim.AdamW(fx.groups(params), fused=False, foreach=False)
    advance = fx.schedulers(ref)
    d_ref, d_norm = np.zeros((fx.steps, len(params), 3)), np.zeros(fx.steps)
    for k in range(fx.steps):
        for i, p in enumerate(params):
            p.grad = fx.gradient(k, i, "cuda")
        norm = torch.nn.utils.clip_grad_norm_(params, fx.max_norm)
        ref.step()
        advance(k)
        d_ref[k], d_norm[k] = fx.distances(k, OC.state_triples(ref, params), float(norm))
    worst = []
    for k, (triples, norm) in enumerate(_fixture_run(fx)):
        fx.check_step(k, triples, float(norm), d_ref=d_ref, d_ref_norm=d_norm, worst=worst)
    print("optimizer vs torch on the device: worst error / bound per step (tensors, norm):", worst)


def _both(shapes, steps, make_grad, max_norm=0.1, lr=1e-2):
    """This class and clip_grad_norm_ + torch.optim.AdamW on copies of the same tensors; returns both parameter lists."""
    torch.manual_seed(3)
    pa = [nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    pb = [nn.Parameter(p.detach().clone()) for p in pa]
    a = ClippedAdamW(pa, lr=lr, max_norm=max_norm)
    b = torch.optim.AdamW(pb, lr=lr, weight_decay=1e-4, fused=False, foreach=False)
    norms = []
    for k in range(steps):
        for i, (p, q) in enumerate(zip(pa, pb)):
            g = make_grad(k, i, p)
            p.grad = g
            q.grad = None if g is None else g.clone()
        if max_norm > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(pb, max_norm))
        b.step()
        a.step()
    return pa, pb, a, b, norms


def _close(x, y, steps):
    """Within three float32 roundings of the largest element per step: the clip coefficient (norm summed in double here,
    in float32 by torch) may differ by one rounding, which the scaled gradient carries once and its square twice; torch's
    device kernels also fuse ``lerp`` into one FMA and divide before scaling in ``addcdiv``, a rounding each."""
    return float((x - y).abs().max()) <= 3 * steps * OC.ulp32(float(y.abs().max()))


def test_clip_inactive_step_is_plain_adamw():
    pa, pb, a, _, norms = _both([(5,), (300, 7)], 2, lambda k, i, p: torch.randn_like(p) * 1e-4)
    assert float(a.last_grad_norm) < 0.1 and abs(float(a.last_grad_norm) - float(norms[-1])) <= 2 ** -22 * float(norms[-1])
    for p, q in zip(pa, pb):
        assert _close(p.detach(), q.detach(), 2)


def test_max_norm_zero_means_no_clip():
    pa, pb, a, _, _ = _both([(5,), (300, 7)], 3, lambda k, i, p: torch.randn_like(p) * 50, max_norm=0.0)
    assert float(a.last_grad_norm) > 100
    for p, q in zip(pa, pb):
        assert _close(p.detach(), q.detach(), 3)


def test_none_gradient_leaves_parameter_and_moments_untouched():
    seen = {}

    def grad(k, i, p):
        if k == 1 and i == 0:
            seen["before"] = p.detach().clone()
            return None
        return torch.randn_like(p)
    pa, pb, a, b, _ = _both([(1030,), (64, 3)], 3, grad)
    # the skipped tensor took two steps, as torch counts them; its moments are those of two steps
    assert float(a.state_dict()["state"][0]["step"]) == 2.0 and float(a.state_dict()["state"][1]["step"]) == 3.0
    for p, q in zip(pa, pb):
        assert _close(p.detach(), q.detach(), 3)
    torch.manual_seed(4)
    p = nn.Parameter(torch.randn(1030, device="cuda"))
    opt = ClippedAdamW([p, nn.Parameter(torch.randn(7, device="cuda"))], lr=1e-2)
    for q in opt.param_groups[0]["params"]:
        q.grad = torch.randn_like(q)
    opt.step()
    before = [t.clone() for t in OC.state_triples(opt, [p])[0]]
    version = p._version
    p.grad = None
    opt.step()
    after = OC.state_triples(opt, [p])[0]
    assert all(torch.equal(x, y) for x, y in zip(before, after)) and p._version == version


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_gives_what_torch_gives(bad):
    def grad(k, i, p):
        g = torch.randn_like(p)
        if k == 1 and i == 1:
            g.view(-1)[3] = bad
        return g
    pa, pb, a, _, norms = _both([(40,), (300, 7)], 2, grad)
    assert not torch.isfinite(a.last_grad_norm) and not torch.isfinite(norms[-1])
    for p, q in zip(pa, pb):
        assert torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(torch.isinf(p), torch.isinf(q))
        finite = torch.isfinite(q)
        assert _close(p.detach()[finite], q.detach()[finite], 2) if finite.any() else True


def test_step_bumps_versions_and_derived_operands_are_rebuilt():
    """The kernels write through raw pointers: without the bump a ``derived()`` operand (here the packed feed-forward
    weights) would stay the one of the old weights."""
    from salience_detr_amd import filter_ops
    torch.manual_seed(0)
    l1, l2, norm = nn.Linear(256, 2048).cuda(), nn.Linear(2048, 256).cuda(), nn.LayerNorm(256).cuda()
    params = list(l1.parameters()) + list(l2.parameters()) + list(norm.parameters())
    old_packed = filter_ops._ffn_operands(l1, l2, norm)[0].clone()
    opt = ClippedAdamW(params, lr=1e-2, max_norm=0.0)
    for p in params:
        p.grad = torch.randn_like(p)
    versions = [p._version for p in params]
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    packed, small = filter_ops._ffn_operands(l1, l2, norm)
    fresh = [copy.deepcopy(m) for m in (l1, l2, norm)]
    want_packed, want_small = filter_ops._ffn_operands(*fresh)
    assert torch.equal(packed, want_packed) and not torch.equal(packed, old_packed)
    assert all(torch.equal(x, y) for x, y in zip(small, want_small))
    # the same through a replayed graph + after_replay()
    for p in params:
        p.grad = torch.randn_like(p)
    opt.prepare()
    torch.cuda.synchronize()
    graph = graph_guard.new_graph()
    with torch.cuda.graph(graph):
        opt.step_captured()
    versions = [p._version for p in params]
    graph.replay()
    opt.after_replay()
    assert all(p._version > v for p, v in zip(params, versions))
    packed = filter_ops._ffn_operands(l1, l2, norm)[0]
    assert torch.equal(packed, filter_ops._ffn_operands(*[copy.deepcopy(m) for m in (l1, l2, norm)])[0])


def test_layouts_match_the_per_tensor_statement():
    """Tensor boundaries, misaligned slices of a flat buffer (parameters AND gradients) and hundreds of tiny tensors next
    to one large tensor, against the same step taken one tensor at a time in plain torch operations on the host."""
    torch.manual_seed(9)
    sizes = [1, 3, 1023, 1024, 1025, 2047, 4099, 5] + [2] * 150 + [7] * 150 + [300 * 1024 + 3]
    flat_p = torch.randn(sum(sizes) + 8, device="cuda")
    flat_g = torch.randn(sum(sizes) + 8, device="cuda") * 0.1
    params, grads, host = [], [], []
    off_p, off_g = 1, 2                      # parameter and gradient slices misaligned, and differently
    for n in sizes:
        p = nn.Parameter(flat_p[off_p:off_p + n])
        params.append(p)
        grads.append(flat_g[off_g:off_g + n])
        host.append(nn.Parameter(p.detach().cpu().clone()))
        off_p, off_g = off_p + n, off_g + n
    guard = flat_p[[0, -7, -6, -5, -4, -3, -2, -1]].clone()
    opt = ClippedAdamW(params, lr=1e-2, max_norm=0.1)
    ref = ClippedAdamW(host, lr=1e-2, max_norm=0.1)      # the plain-torch statement, tensor by tensor
    for k in range(2):
        for p, g, h in zip(params, grads, host):
            p.grad = g
            h.grad = g.cpu().clone()
        opt.step()
        ref.step()
        flat_g.mul_(0.5)
    torch.cuda.synchronize()
    assert torch.equal(flat_p[[0, -7, -6, -5, -4, -3, -2, -1]], guard)       # nothing written outside the slices
    assert abs(float(opt.last_grad_norm) - float(ref.last_grad_norm)) <= 2 ** -22 * float(ref.last_grad_norm)
    for p, h, (m, v), (hm, hv) in zip(params, host, opt._views, ref._views):
        assert _close(p.detach().cpu(), h.detach(), 2) and _close(m.cpu(), hm, 2) and _close(v.cpu(), hv, 2)


def test_reducer_gradients_through_the_kernels():
    """``from_reducer`` on the device: the gradients are the slices of a ``StaticGradAllReducer``'s flat buffer (odd-sized
    tensors in front misalign them against their parameters) and ``grad_scale`` folds an average in; against
    ``clip_grad_norm_`` + ``torch.optim.AdamW`` on the scaled gradients.  One process: no process group is needed."""
    from salience_detr_amd.data_parallel import StaticGradAllReducer
    torch.manual_seed(12)
    shapes = [(3,), (257, 5), (1,), (2048, 3), (1030,), (7, 7)]
    pa = [nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    pb = [nn.Parameter(p.detach().clone()) for p in pa]
    red = StaticGradAllReducer(pa)
    opt = ClippedAdamW.from_reducer(red, lr=1e-2, max_norm=0.1, grad_scale=0.5)      # as if two ranks had been summed
    ref = torch.optim.AdamW(pb, lr=1e-2, weight_decay=1e-4, fused=False, foreach=False)
    assert any(v.data_ptr() % 16 != p.data_ptr() % 16 for v, p in zip(red.views, pa))
    for k in range(3):
        for p, q in zip(pa, pb):
            p.grad = torch.randn_like(p) * (0.3 if k else 1e-3)       # the first step's norm is below max_norm
            q.grad = p.grad * 0.5
        red.pack()
        red.all_reduce(average=False)
        versions = [p._version for p in pa]
        opt.step()
        assert all(p._version > v for p, v in zip(pa, versions))
        norm = torch.nn.utils.clip_grad_norm_(pb, 0.1)
        ref.step()
        assert abs(float(opt.last_grad_norm) - float(norm)) <= 2 ** -22 * float(norm)
    for p, q in zip(pa, pb):
        assert _close(p.detach(), q.detach(), 3)


def _detector_setup(static_proposals=False):
    import detector_train_cases as DT
    case = DT.Case("small")
    det = case.detector([m.cuda() for m in case.stored_maps()]).cuda().train()
    det.transformer.static_proposals = static_proposals
    images = [torch.zeros(3, h, w).cuda() for h, w in case.sizes]
    return case, det, images, case.targets(), case.noise().cuda()


def _trajectory(kind, static_proposals=False):
    from salience_detr_amd.optimizer import param_groups
    case, det, images, targets, noise = _detector_setup(static_proposals)
    groups = param_groups(det, 1e-4)
    opt = ClippedAdamW(groups, lr=1e-4, max_norm=0.1) if kind == "hip" else \
        torch.optim.AdamW(groups, lr=1e-4, weight_decay=1e-4, fused=False, foreach=False)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = sum(det(images, targets, noise=noise).values())
        loss.backward()
        if kind != "hip":
            torch.nn.utils.clip_grad_norm_(det.parameters(), 0.1)
        opt.step()
        losses.append(float(loss))
    return losses


def test_four_detector_training_steps_match_torch_adamw():
    """Forward + backward of the detector on ``detector_train_small.npz`` + this optimizer, four steps, against the same
    steps with ``clip_grad_norm_`` + ``torch.optim.AdamW``: the same loss trajectory within 1e-4."""
    got, want = _trajectory("hip"), _trajectory("torch")
    print("detector loss trajectory:", got, want)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)


def test_four_detector_training_steps_as_one_graph():
    """The same four steps as ONE captured graph: forward + backward + ``step_captured()``, replayed four times with
    ``after_replay()`` between the replays, against ``clip_grad_norm_`` + ``torch.optim.AdamW`` run eagerly: the same loss
    trajectory within 1e-4.  Everything that comes from the host is staged before the capture (images batched, targets
    prepared and staged, the salience criterion's boxes); the gradients sit at fixed addresses
    (``zero_grad(set_to_none=False)`` is the region's first call) and ``prepare(whole_step=True)`` makes the operands
    derived from the weights stale, so that they are rebuilt inside the graph: a replay that read operands of the weights
    before the first step would leave the trajectory of the eager steps.  The proposal count is not read back
    (``static_proposals``), on both sides."""
    from salience_detr_amd.backbone import batch_images
    from salience_detr_amd.detector import prepare_targets
    from salience_detr_amd.optimizer import param_groups
    from salience_detr_amd.set_criterion import stage_targets
    want = _trajectory("torch", static_proposals=True)

    case, det, images, targets, noise = _detector_setup(static_proposals=True)
    opt = ClippedAdamW(param_groups(det, 1e-4), lr=1e-4, max_norm=0.1)
    with torch.no_grad():
        canvas, mask = batch_images(images, normalize=False)
    prepared = prepare_targets(targets, case.sizes)
    staged = stage_targets(prepared, device="cuda")
    focus = det.focus_criterion.stage_boxes(prepared, case.sizes, "cuda")
    size = tuple(canvas.shape[-2:])

    def whole_step(last):
        opt.zero_grad(set_to_none=False)
        loss = sum(det.forward_train(det.backbone(canvas), mask, prepared, case.sizes, size, noise=noise, staged=staged,
                                     focus_boxes=focus).values())
        loss.backward()
        last()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        whole_step(lambda: None)            # forward + backward only: the gradients exist, the weights are untouched
    torch.cuda.current_stream().wait_stream(side)
    first = float(whole_step(lambda: None))  # (still the weights of step 0)
    opt.prepare(whole_step=True)
    torch.cuda.synchronize()
    graph = graph_guard.new_graph()
    with torch.cuda.graph(graph):
        loss = whole_step(opt.step_captured)
    types = graph_guard.node_types(graph)
    assert types, "no graph handle: the memset check could not be made"
    print("captured training step with the optimizer:", graph_guard.assert_replay_safe(graph, "whole training step"), "nodes")
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    got = []
    for _ in range(4):
        versions = [p._version for p in params]
        graph.replay()
        got.append(float(loss))
        opt.after_replay()
        assert all(p._version > v for p, v in zip(params, versions))
    print("detector loss trajectory, one graph per step:", got, want)
    assert abs(first - want[0]) <= 1e-4 * max(1.0, abs(want[0]))
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)
    assert abs(want[-1] - want[0]) > 1e-4 * max(1.0, abs(want[0])), want
    assert float(opt.state_dict()["state"][0]["step"]) == 4
