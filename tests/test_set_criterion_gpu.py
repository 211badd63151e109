"""GPU: the set criterion (salience_detr_amd/set_criterion.py, csrc/set_criterion.hip) against the imported reference's
HybridSetCriterion / HungarianMatcher / compute_dn_loss (tests/golden/set_criterion_cases.npz, see
make_set_criterion_golden.py), a torch restatement of the cost, an optimality certificate from the kernel's fp64 duals,
brute force on small problems, a float64 autograd restatement of the loss, and graph replay."""
import itertools
import os

import numpy as np
import pytest
import torch

from salience_detr_amd import set_criterion as S

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
C = 91
KEYS = ("loss_class", "loss_bbox", "loss_giou")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "set_criterion_cases.npz"))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def draw_full(seed, B=2, Nq=900, n_out=7, counts=(20, 100)):
    """make_set_criterion_golden.draw_full: the full-size case's inputs from torch's CPU generator."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(n_out, B, Nq, C, generator=g) * 1.5 - 3.0).half().float()
    cxcy = torch.rand(n_out, B, Nq, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n_out, B, Nq, 2, generator=g) * 0.3 + 0.02
    boxes = torch.cat([cxcy, wh], -1)
    targets = []
    for n in counts:
        tc = torch.rand(n, 2, generator=g) * 0.8 + 0.1
        tw = torch.rand(n, 2, generator=g) * 0.3 + 0.02
        targets.append({"boxes": torch.cat([tc, tw], -1), "labels": torch.randint(0, C, (n,), generator=g)})
    return logits, boxes, targets


def case_inputs(gold, tag, dtype=None):
    if tag == "full":
        logits, boxes, targets = draw_full(int(gold["full_seed"][0]))
        digest = [logits.double().sum().item(), boxes.double().sum().item(),
                  sum(t["boxes"].double().sum().item() for t in targets)]
        np.testing.assert_allclose(digest, gold["full_input_digest"], rtol=0, atol=0)
        return logits.to(dtype or torch.float32), boxes, targets
    if f"{tag}_logits_bf16" in gold.files:
        logits = _t(gold[f"{tag}_logits_bf16"]).view(torch.bfloat16)
    else:
        logits = _t(gold[f"{tag}_logits_f16"]).float()
    if dtype is not None:
        logits = logits.to(dtype)
    counts = gold[f"{tag}_counts"].tolist()
    tb, tl = _t(gold[f"{tag}_tboxes"]), _t(gold[f"{tag}_tlabels"]).long()
    targets, o = [], 0
    for n in counts:
        targets.append({"boxes": tb[o:o + n], "labels": tl[o:o + n]})
        o += n
    return logits, _t(gold[f"{tag}_boxes"]), targets


def outputs_of(lg, bx, enc=True):
    n = lg.shape[0]
    dec = n - 1 if enc else n
    out = {"pred_logits": lg[0], "pred_boxes": bx[0],
           "aux_outputs": [{"pred_logits": lg[i], "pred_boxes": bx[i]} for i in range(1, dec)]}
    if enc:
        out["enc_outputs"] = {"pred_logits": lg[n - 1], "pred_boxes": bx[n - 1]}
    return out


def suffixes(n):
    return [""] + [f"_{i}" for i in range(n - 2)] + ["_enc"]


def criterion(binary=False):
    return S.HybridSetCriterion(C, S.HungarianMatcher(2, 5, 2), {}, alpha=0.25, gamma=2.0, two_stage_binary_cls=binary)


def to_dev(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def close(got, ref, rtol, atol=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(got - ref) > rtol * np.abs(ref) + atol
    assert not bad.any(), (f"{bad.sum()} of {bad.size} outside {rtol} rel + {atol} abs; worst "
                           f"{np.max(np.abs(got - ref) - rtol * np.abs(ref)):.3e}")


def run(gold, tag, dtype=None):
    """(match [n, B, Nq], losses [n, 3], grad_logits, grad_boxes) of the criterion on case `tag`."""
    logits, boxes, targets = case_inputs(gold, tag, dtype)
    n_out = logits.shape[0]
    binary = bool(gold[f"{tag}_shape"][4])
    crit = criterion(binary)
    lg = logits.to(DEV).requires_grad_(True)
    bx = boxes.to(DEV).requires_grad_(True)
    tg = to_dev(targets)
    staged = S.stage_targets(tg)
    match = crit.matcher.match([lg[i] for i in range(n_out)], [bx[i] for i in range(n_out)], staged,
                               [False] * (n_out - 1) + [binary])[0]
    losses = crit(outputs_of(lg, bx), tg, staged=staged)
    sfx = suffixes(n_out)
    assert set(losses) == {k + s for s in sfx for k in KEYS}
    w = _t(gold[f"{tag}_weights"]).to(DEV)
    total = sum(w[i, k] * losses[KEYS[k] + s] for i, s in enumerate(sfx) for k in range(3))
    total.backward()
    L = torch.stack([torch.stack([losses[k + s] for k in KEYS]) for s in sfx])
    B, Nq = logits.shape[1:3]
    return (match.view(n_out, B, Nq).cpu().numpy(), L.detach().cpu().numpy(), lg.grad.float().cpu().numpy(),
            bx.grad.cpu().numpy())


@pytest.mark.parametrize("tag", ["main", "empty", "binary", "full"])
def test_parity_with_reference(gold, tag):
    match, losses, gl, gb = run(gold, tag)
    np.testing.assert_array_equal(match, gold[f"{tag}_match"])
    close(losses, gold[f"{tag}_losses"], 1e-5)
    if f"{tag}_grad_logits" in gold.files:
        close(gl, gold[f"{tag}_grad_logits"], 1e-5, 1e-7)
    if f"{tag}_grad_logits0" in gold.files:
        close(gl[0], gold[f"{tag}_grad_logits0"], 1e-5, 1e-7)
    # digests: sums of up to 91 (row) / 900 (column) gradients, each within the element bar
    close(gl.astype(np.float64).sum(-1), gold[f"{tag}_grad_logits_rowsum"], 1e-5, 91e-7)
    close(gl.astype(np.float64).sum(-2), gold[f"{tag}_grad_logits_colsum"], 1e-5, gl.shape[-2] * 1e-7)
    if f"{tag}_grad_boxes" in gold.files:
        close(gb, gold[f"{tag}_grad_boxes"], 1e-5, 1e-7)
    else:
        close(gb.astype(np.float64).sum(2), gold[f"{tag}_grad_boxes_sum"], 1e-5, gb.shape[2] * 1e-7)


def test_bf16_logits(gold):
    """bf16 logits, main library: the reference ran on the same values upcast to fp32.  Indices and losses at the fp32 bars
    (the kernel reads the same values); d/dlogits is stored in bf16 (8 mantissa bits)."""
    match, losses, gl, gb = run(gold, "bf16")
    np.testing.assert_array_equal(match, gold["bf16_match"])
    close(losses, gold["bf16_losses"], 1e-5)
    close(gb, gold["bf16_grad_boxes"], 1e-5, 1e-7)
    close(gl.astype(np.float64).sum(-1), gold["bf16_grad_logits_rowsum"], 1e-2, 91 * 1e-6)


def test_fp16_logits_f16_library(gold):
    """fp16 logits go to the fp16-activation library; the main case's logits are fp16-representable, so indices and
    losses hold at the fp32 bars."""
    match, losses, gl, gb = run(gold, "main", torch.float16)
    np.testing.assert_array_equal(match, gold["main_match"])
    close(losses, gold["main_losses"], 1e-5)
    close(gb, gold["main_grad_boxes"], 1e-5, 1e-7)
    close(gl[0], gold["main_grad_logits0"], 2e-3, 1e-6)


def test_dn_loss(gold):
    groups, max_gt, nq, n_out = gold["dn_params"].tolist()
    logits, boxes = _t(gold["dn_logits_f16"]).float(), _t(gold["dn_boxes"])
    counts = gold["dn_counts"].tolist()
    tb, tl = _t(gold["dn_tboxes"]), _t(gold["dn_tlabels"]).long()
    tg = to_dev([{"boxes": tb[:counts[0]], "labels": tl[:counts[0]]},
                 {"boxes": tb[counts[0]:], "labels": tl[counts[0]:]}])
    staged = S.stage_targets(tg)
    match, status = S.dn_match(staged, nq, groups, max_gt, n_out)
    assert (status == 0).all()
    for o in range(n_out):
        np.testing.assert_array_equal(match.view(n_out, 2, nq)[o].cpu().numpy(), gold["dn_match"])
    # the DN outputs as [:, :pad] query slices of a larger decoder output, as dn_post_process leaves them
    big_l = torch.randn(n_out, 2, nq + 50, C, device=DEV)
    big_b = torch.rand(n_out, 2, nq + 50, 4, device=DEV)
    big_l[:, :, :nq] = logits.to(DEV)
    big_b[:, :, :nq] = boxes.to(DEV)
    big_l.requires_grad_(True)
    big_b.requires_grad_(True)
    dn_out = {"pred_logits": big_l[0, :, :nq], "pred_boxes": big_b[0, :, :nq],
              "aux_outputs": [{"pred_logits": big_l[i, :, :nq], "pred_boxes": big_b[i, :, :nq]} for i in range(1, n_out)]}
    losses = criterion().dn_losses(dn_out, tg, groups, max_gt, staged=staged)
    sfx = ["_dn"] + [f"_dn_{i}" for i in range(n_out - 1)]
    L = np.array([[losses[k + s].item() for k in KEYS] for s in sfx])
    close(L, gold["dn_losses"], 1e-5)
    w = _t(gold["dn_weights"]).to(DEV)
    sum(w[i, k] * losses[KEYS[k] + s] for i, s in enumerate(sfx) for k in range(3)).backward()
    close(big_l.grad[:, :, :nq].cpu().numpy(), gold["dn_grad_logits"], 1e-5, 1e-7)
    close(big_b.grad[:, :, :nq].cpu().numpy(), gold["dn_grad_boxes"], 1e-5, 1e-7)
    assert not big_l.grad[:, :, nq:].any() and not big_b.grad[:, :, nq:].any()


def test_per_image_matcher_and_calculate_loss(gold):
    logits, boxes, targets = case_inputs(gold, "main")
    matcher = S.HungarianMatcher(2, 5, 2)
    indices = []
    for b, t in enumerate(to_dev(targets)):
        src, tgt = matcher(boxes[0, b].to(DEV), logits[0, b].to(DEV), t["boxes"], t["labels"])
        assert src.dtype == torch.int64 and tgt.dtype == torch.int64 and bool((src[1:] > src[:-1]).all())
        ref = gold["main_match"][0, b]
        np.testing.assert_array_equal(src.cpu().numpy(), np.nonzero(ref >= 0)[0])
        np.testing.assert_array_equal(tgt.cpu().numpy(), ref[ref >= 0])
        indices.append((src, tgt))
    crit = S.HybridSetCriterion(C, matcher, {})
    out = {"pred_logits": logits[0].to(DEV), "pred_boxes": boxes[0].to(DEV)}
    nb = float(max(sum(gold["main_counts"]), 1))
    got = crit.calculate_loss(out, to_dev(targets), nb, indices=indices)
    close([got[k].item() for k in KEYS], gold["main_losses"][0], 1e-5)
    got2 = crit.calculate_loss(out, to_dev(targets), torch.tensor(nb, device=DEV))
    close([got2[k].item() for k in KEYS], gold["main_losses"][0], 1e-5)


# ---- cost and assignment -------------------------------------------------------------------------------------------
def torch_cost(logits, boxes, tboxes, labels, wc=2.0, wb=5.0, wg=2.0, alpha=0.25, gamma=2.0):
    """hungarian_matcher.py:41-71 restated in torch (fp32, on the device): [Nq, T]."""
    p = logits.float().sigmoid()
    neg = -(1 - alpha) * p ** gamma * (1 - p + 1e-6).log()
    pos = -alpha * (1 - p) ** gamma * (p + 1e-6).log()
    cls = pos[:, labels] - neg[:, labels]
    l1 = torch.cdist(boxes, tboxes, p=1)

    def xyxy(b):
        cx, cy, w, h = b.unbind(-1)
        return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)

    a, b = xyxy(boxes), xyxy(tboxes)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b - inter
    ewh = (torch.max(a[:, None, 2:], b[:, 2:]) - torch.min(a[:, None, :2], b[:, :2])).clamp(min=0)
    area_c = ewh[..., 0] * ewh[..., 1]
    giou = inter / union - (area_c - union) / area_c
    return wb * l1 + wc * cls + wg * (-giou)


def random_problem(seed, Nq, counts, dup=False):
    g = torch.Generator().manual_seed(seed)
    B = len(counts)
    logits = torch.randn(B, Nq, C, generator=g) * 1.5 - 3.0
    boxes = torch.cat([torch.rand(B, Nq, 2, generator=g) * 0.8 + 0.1, torch.rand(B, Nq, 2, generator=g) * 0.3 + 0.02], -1)
    targets = []
    for n in counts:
        tb = torch.cat([torch.rand(n, 2, generator=g) * 0.8 + 0.1, torch.rand(n, 2, generator=g) * 0.3 + 0.02], -1)
        tl = torch.randint(0, C, (n,), generator=g)
        if dup and n >= 2:       # ties: identical targets and identical queries
            tb[1], tl[1] = tb[0], tl[0]
        targets.append({"boxes": tb, "labels": tl})
    if dup and Nq >= 2:
        logits[:, 1], boxes[:, 1] = logits[:, 0], boxes[:, 0]
    return logits.to(DEV), boxes.to(DEV), to_dev(targets)


def solve(logits, boxes, targets, capacity=None):
    staged = S.stage_targets(targets, capacity)
    match, status, duals, cost = S.match_outputs([logits], [boxes], staged, 2, 5, 2, 0.25, 2.0, with_duals=True,
                                                 with_cost=True)
    return staged, match.cpu(), status.cpu(), duals.cpu(), cost.cpu()


def certify(match, duals, cost, T, Nq):
    """Dual feasibility + complementary slackness of min sum c over assignments of every row (target) to a distinct
    column (query): c - u - v >= 0, == 0 on matched pairs, v <= 0, v == 0 on unmatched columns."""
    m = match.numpy()
    assigned = m[m >= 0]
    assert sorted(assigned.tolist()) == list(range(T)), "every target matched once"
    if T == 0:
        return
    c = cost[:T].double().numpy()            # [T, Nq]
    v, u = duals[:Nq].numpy(), duals[Nq:Nq + T].numpy()
    red = c - u[:, None] - v[None, :]
    tol = 1e-9 * max(1.0, np.abs(c).max()) * max(T, 1)
    assert red.min() >= -tol, red.min()
    q = np.nonzero(m >= 0)[0]
    assert np.abs(red[m[q], q]).max() <= tol
    assert v.max() <= tol
    free = m < 0
    if free.any():
        assert np.abs(v[free]).max() <= tol


@pytest.mark.parametrize("Nq,counts,dup", [(50, (1, 0), False), (1, (1, 0), False), (1, (0, 0), False),
                                           (40, (40, 17), False), (900, (300, 100), False), (60, (12, 30), True),
                                           (8, (8, 8), True)])
def test_optimality_certificate(Nq, counts, dup):
    logits, boxes, targets = random_problem(100 + Nq + sum(counts), Nq, counts, dup)
    staged, match, status, duals, cost = solve(logits, boxes, targets)
    assert (status == 0).all()
    for b, T in enumerate(counts):
        certify(match[b], duals[b], cost[b], T, Nq)
        if T:
            ref = torch_cost(logits[b], boxes[b], targets[b]["boxes"], targets[b]["labels"]).t().cpu()
            got = cost[b, :T]
            assert ((got - ref).abs() <= 1e-6 * ref.abs().clamp(min=1)).all()


def test_cost_against_torch():
    logits, boxes, targets = random_problem(7, 300, (37, 5))
    _, _, _, _, cost = solve(logits, boxes, targets, capacity=40)
    for b, t in enumerate(targets):
        ref = torch_cost(logits[b], boxes[b], t["boxes"], t["labels"]).t().cpu()
        T = ref.shape[0]
        assert ((cost[b, :T] - ref).abs() <= 1e-6 * ref.abs().clamp(min=1)).all()


def test_brute_force_small():
    for seed in range(12):
        Nq = 1 + seed % 7
        T = min(Nq, 1 + seed % 4)
        logits, boxes, targets = random_problem(1000 + seed, Nq, (T,))
        _, match, status, _, cost = solve(logits, boxes, targets)
        assert int(status[0]) == 0
        c = cost[0, :T].double().numpy()
        best = min(sum(c[t, perm[t]] for t in range(T)) for perm in itertools.permutations(range(Nq), T))
        m = match[0].numpy()
        got = sum(c[m[q], q] for q in range(Nq) if m[q] >= 0)
        assert abs(got - best) <= 1e-9 * max(1.0, abs(best))


def test_scipy_agrees():
    scipy_opt = pytest.importorskip("scipy.optimize")
    logits, boxes, targets = random_problem(31, 900, (100, 20))
    _, match, status, _, cost = solve(logits, boxes, targets)
    for b, T in enumerate((100, 20)):
        c = cost[b, :T].double().numpy()
        rows, cols = scipy_opt.linear_sum_assignment(c)
        m = match[b].numpy()
        got = sum(c[m[q], q] for q in range(900) if m[q] >= 0)
        assert abs(got - c[rows, cols].sum()) <= 1e-9 * abs(c[rows, cols].sum())


def test_status_for_over_capacity_and_dn_overflow():
    logits, boxes, targets = random_problem(5, 20, (3, 4))
    staged = S.stage_targets(targets, capacity=4)
    small = staged._replace(capacity=3)      # a capacity below an image's count: that problem reports 2
    match, status = S.match_outputs([logits], [boxes], small, 2, 5, 2, 0.25, 2.0)
    assert status.tolist() == [0, 2] and (match[1] == -1).all()
    m, st = S.dn_match(staged, 20, 5, 3)
    assert st.tolist() == [0, 2]


# ---- gradients against a float64 restatement ------------------------------------------------------------------------
def restated_loss(logits, boxes, tb, tl, offsets, match, nb, alpha=0.25, gamma=2.0):
    """vari_sigmoid_focal_loss + L1 + GIoU in float64 for a given match [B, Nq]; weight and target score detached."""
    B, Nq, Cc = logits.shape
    x = logits.double()
    bx = boxes.double()
    q_idx, b_idx, t_idx = [], [], []
    for b in range(B):
        q = torch.nonzero(match[b] >= 0).flatten()
        q_idx.append(q)
        b_idx.append(torch.full_like(q, b))
        t_idx.append(match[b][q].long() + int(offsets[b]))
    q_idx, b_idx, t_idx = torch.cat(q_idx), torch.cat(b_idx), torch.cat(t_idx)
    src, tgt = bx[b_idx, q_idx], tb.double()[t_idx]

    def xyxy(b):
        cx, cy, w, h = b.unbind(-1)
        return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)

    a, t = xyxy(src), xyxy(tgt)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_t = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    wh = (torch.min(a[:, 2:], t[:, 2:]) - torch.max(a[:, :2], t[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area_a + area_t - inter
    ewh = (torch.max(a[:, 2:], t[:, 2:]) - torch.min(a[:, :2], t[:, :2])).clamp(min=0)
    area_c = ewh[:, 0] * ewh[:, 1]
    iou = inter / union
    giou = iou - (area_c - union) / area_c
    onehot = torch.zeros_like(x)
    onehot[b_idx, q_idx, tl[t_idx].long()] = 1.0
    score = torch.zeros_like(x)
    score[b_idx, q_idx, tl[t_idx].long()] = iou.detach()
    prob = x.sigmoid().detach()
    w = (1 - alpha) * prob ** gamma * (1 - onehot) + score
    cls = torch.nn.functional.binary_cross_entropy_with_logits(x, score, weight=w, reduction="sum") / nb
    l1 = (src - tgt).abs().sum() / nb
    lg = (1 - giou).sum() / nb
    return torch.stack([cls, l1, lg])


def test_gradients_against_float64_restatement():
    logits, boxes, targets = random_problem(77, 300, (9, 31))
    staged = S.stage_targets(targets)
    lg = logits.clone().requires_grad_(True)
    bx = boxes.clone().requires_grad_(True)
    match = S.match_outputs([lg], [bx], staged, 2, 5, 2, 0.25, 2.0)[0]
    out = S.set_losses([lg], [bx], staged, match)
    w = torch.tensor([[1.3, 0.7, 1.9]], device=DEV)
    (out * w).sum().backward()
    l64 = logits.double().clone().requires_grad_(True)
    b64 = boxes.double().clone().requires_grad_(True)
    ref = restated_loss(l64, b64, staged.boxes, staged.labels, staged.offsets.cpu(), match, 40.0)
    (ref * w[0].double()).sum().backward()
    close(out.detach().cpu().numpy()[0], ref.detach().cpu().numpy(), 1e-5)
    close(lg.grad.cpu().numpy(), l64.grad.cpu().numpy(), 1e-5, 1e-7)
    close(bx.grad.cpu().numpy(), b64.grad.cpu().numpy(), 1e-5, 1e-7)


# ---- graph capture --------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager():
    cap = 40
    logits, boxes, t1 = random_problem(11, 300, (12, 33))
    _, _, t2 = random_problem(12, 300, (40, 3))
    n_out = 3
    lg = torch.stack([logits + 0.1 * i for i in range(n_out)]).requires_grad_(True)
    bx = torch.stack([boxes] * n_out).requires_grad_(True)
    crit = criterion()
    w = torch.linspace(0.5, 1.5, 3 * n_out, device=DEV).view(n_out, 3)

    def step(staged):
        losses = crit(outputs_of(lg, bx), None, staged=staged)
        L = torch.stack([torch.stack([losses[k + s] for k in KEYS]) for s in suffixes(n_out)])
        gl, gb = torch.autograd.grad((L * w).sum(), [lg, bx])
        return L, gl, gb

    staged = S.stage_targets(t1, capacity=cap)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(staged)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L_g, gl_g, gb_g = step(staged)
    for targets in (t2, t1):
        staged.copy_(S.stage_targets(targets, capacity=cap))
        graph.replay()
        L_e, gl_e, gb_e = step(S.stage_targets(targets, capacity=cap))
        torch.cuda.synchronize()
        assert torch.equal(L_g, L_e) and torch.equal(gl_g, gl_e) and torch.equal(gb_g, gb_e)
