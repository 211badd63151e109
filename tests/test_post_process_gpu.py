"""GPU: detection post-processing (salience_detr_amd/post_process.py, csrc/post_process.hip) against the reference's
PostProcess outputs (tests/golden/postprocess_cases.npz, see make_postprocess_golden.py), a CPU stable-sort oracle and
the oracle's greedy NMS."""
import os

import numpy as np
import pytest
import torch

from oracle import salience_ref as R
from salience_detr_amd import graph_guard
from salience_detr_amd.post_process import PostProcess, detections_padded

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "postprocess_cases.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def oracle(logits, boxes, sizes, k):
    """Top k by logit descending, equal logits in flat-index order (a stable sort), then the reference's epilogue in
    torch on CPU.  Returns (scores in the logits' dtype, labels, boxes)."""
    B, Nq, C = logits.shape
    flat = logits.reshape(B, -1)
    order = torch.sort(-flat.float(), dim=1, stable=True)[1][:, :k]
    scores = torch.gather(flat, 1, order).sigmoid()
    labels = order % C
    q = torch.div(order, C, rounding_mode="trunc")
    b = boxes[torch.arange(B)[:, None], q]
    cx, cy, w, h = b.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    img_h, img_w = sizes.unbind(1)
    scale = torch.stack([img_w, img_h, img_w, img_h], 1)
    return scores, labels, xyxy * scale[:, None, :]


def run(logits, boxes, sizes, k, conf=-1, nms=-1):
    out = detections_padded(logits.cuda(), boxes.cuda(), sizes.cuda(), k, conf, nms)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


# The kernel computes torch's fp32 formula 1 / (1 + exp(-x)) with the device expf; CPU ATen's vectorised sigmoid evaluates
# the same formula with SLEEF's expf.  Neither exp is correctly rounded and they differ by up to 2 ulps of the score on the
# fixture (selection, labels and boxes are bit-exact).
SCORE_ULPS = 2.0


def ulps(a, b):
    """|a - b| in units of b's spacing (fp32 compare of values held in any float dtype)."""
    a, b = a.float().numpy(), b.float().numpy()
    return np.abs(a - b) / np.spacing(np.abs(b).astype(np.float32))


def check_padding(s, l, b, count, k):
    for i, c in enumerate(count.tolist()):
        assert (s[i, c:].float() == 0).all() and (l[i, c:] == -1).all() and (b[i, c:] == 0).all()


def rand_inputs(B, Nq, C, dtype=torch.float32, seed=0, sizes_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, Nq, C, generator=g) * 1.2 - 4.5).to(dtype)
    boxes = torch.cat([torch.rand(B, Nq, 2, generator=g) * 0.8 + 0.1, torch.rand(B, Nq, 2, generator=g) * 0.3 + 0.02], -1)
    sizes = torch.stack([torch.randint(300, 1400, (B,), generator=g), torch.randint(300, 1400, (B,), generator=g)], 1)
    return logits, boxes.float().contiguous(), sizes.to(sizes_dtype)


# ---- fixture parity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["f32_k100", "f32_k300", "f32_k300_conf", "f32_k300_nms_conf"])
def test_reference_fixture_fp32(gold, tag):
    k, nms, conf = gold[f"{tag}_params"].tolist()
    logits, boxes, sizes = _t(gold["logits_f32"]), _t(gold["boxes"]), _t(gold["target_sizes"])
    s, l, b, count = run(logits, boxes, sizes, int(k), conf, nms)
    for i in range(2):
        ws, wl, wb = gold[f"{tag}_scores{i}"], gold[f"{tag}_labels{i}"], gold[f"{tag}_boxes{i}"]
        c = len(ws)
        assert int(count[i]) == c
        assert np.array_equal(l[i, :c].numpy(), wl)
        assert np.array_equal(b[i, :c].numpy().view(np.uint32), wb.view(np.uint32))
        assert ulps(s[i, :c], _t(ws)).max() <= SCORE_ULPS
    check_padding(s, l, b, count, int(k))
    # the module form returns the reference's structure
    res = PostProcess(int(k), nms, conf)({"pred_logits": logits.cuda(), "pred_boxes": boxes.cuda()}, sizes.cuda())
    assert len(res) == 2
    for i, r in enumerate(res):
        assert set(r) == {"scores", "labels", "boxes"}
        assert r["scores"].dtype == torch.float32 and r["labels"].dtype == torch.int64 and r["boxes"].dtype == torch.float32
        assert np.array_equal(r["labels"].cpu().numpy(), gold[f"{tag}_labels{i}"])
        assert np.array_equal(r["boxes"].cpu().numpy(), gold[f"{tag}_boxes{i}"])


def test_reference_fixture_bf16_is_tie_aware(gold):
    logits = _t(gold["logits_bf16_bits"]).view(torch.bfloat16)
    boxes, sizes = _t(gold["boxes"]), _t(gold["target_sizes"])
    s, l, b, count = run(logits, boxes, sizes, 300)
    assert s.dtype == torch.bfloat16 and count.tolist() == [300, 300]
    prob = logits.reshape(2, -1).sigmoid()
    for i in range(2):
        ref_s = _t(gold[f"bf16_k300_scores{i}"])
        kth = ref_s[-1]
        # every entry strictly above the k-th probability is selected; the remaining slots equal the k-th
        above = torch.nonzero(prob[i].float() > kth)[:, 0]
        ls = l[i].tolist()
        order = torch.sort(-logits[i].reshape(-1).float(), stable=True)[1][:300]
        got_flat = set(order.tolist())
        assert set(above.tolist()) <= got_flat
        assert ls == (order % 91).tolist()
        sp = s[i].float()
        assert (sp[1:] <= sp[:-1]).all()
        assert (sp[len(above):] == kth).all()
        assert torch.equal(sp, ref_s)          # the score sequence itself is order-free inside a tie group
        # descending logit order, equal logits in flat-index order
        lg = logits[i].reshape(-1)[order].float()
        assert (lg[1:] <= lg[:-1]).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_logits_match_stable_sort_oracle(dtype):
    logits, boxes, sizes = rand_inputs(2, 900, 91, dtype, seed=3)
    s, l, b, count = run(logits, boxes, sizes, 300)
    os_, ol, ob = oracle(logits, boxes, sizes, 300)
    assert s.dtype == dtype and count.tolist() == [300, 300]
    assert torch.equal(l, ol) and torch.equal(b, ob)
    assert ulps(s, os_).max() <= SCORE_ULPS
    prob = logits.reshape(2, -1).sigmoid().float()
    for i in range(2):
        kth = os_[i, -1].float()
        assert int((prob[i] > kth).sum()) <= 300
        sp = s[i].float()
        assert (sp[1:] <= sp[:-1]).all()


def test_exact_ties_lowest_flat_index_wins():
    """Logits quantised to 1/8: the k-th place falls inside a large group of equal logits."""
    g = torch.Generator().manual_seed(11)
    logits = torch.round(torch.randn(2, 300, 91, generator=g) * 8) / 8 - 3.0
    _, boxes, sizes = rand_inputs(2, 300, 91, seed=11)
    for k in (100, 300, 1024):
        s, l, b, count = run(logits, boxes, sizes, k)
        os_, ol, ob = oracle(logits, boxes, sizes, k)
        kth = torch.sort(-logits.reshape(2, -1), dim=1, stable=True)[0][:, k - 1]
        assert ((logits.reshape(2, -1) == -kth[:, None]).sum(1) > 10).all()    # a large tie group at the cut
        assert torch.equal(l, ol) and torch.equal(b, ob)
        assert ulps(s, os_).max() <= SCORE_ULPS


# ---- filters -------------------------------------------------------------------------------------------------------

def expected_filtered(s, b, conf, nms):
    """Reference semantics on the build's own (unfiltered) top k: NMS over all k boxes in rank order AND the confidence
    mask (score > conf in the score's dtype)."""
    k = s.shape[0]
    keep = torch.ones(k, dtype=torch.bool)
    if conf > 0:
        keep &= s > conf
    if nms > 0:
        kept = R.nms_greedy(b, -torch.arange(k, dtype=torch.float32), nms)   # rank order
        m = torch.zeros(k, dtype=torch.bool)
        m[kept] = True
        keep &= m
    return torch.nonzero(keep)[:, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nms,conf", [(0.5, 0.3), (0.7, 0.3), (0.5, -1), (-1, 0.3), (0.7, -1)])
def test_nms_and_confidence_against_greedy_nms(dtype, nms, conf):
    B, Nq, C = 2, 400, 91
    logits, _, sizes = rand_inputs(B, Nq, C, dtype, seed=5)
    g = torch.Generator().manual_seed(6)
    base = torch.rand(B, 30, 4, generator=g)
    pick = torch.randint(0, 30, (B, Nq), generator=g)
    bb = torch.gather(base, 1, pick[..., None].expand(-1, -1, 4))
    boxes = torch.cat([bb[..., :2] * 0.8 + 0.1 + torch.randn(B, Nq, 2, generator=g) * 0.01,
                       bb[..., 2:] * 0.3 + 0.03], -1).float().contiguous()
    # a logit whose score is exactly the threshold rounded to the score's dtype (bf16(0.3) = 0.30078125 is not > 0.3)
    x = torch.logit(torch.tensor(0.3, dtype=torch.float64).to(dtype).double()).to(dtype)
    logits = logits.clone()
    logits[:, ::7, 3] = x
    u, ul, ub, _ = run(logits, boxes, sizes, 300)
    assert (u.to(dtype) == torch.tensor(0.3, dtype=torch.float64).to(dtype)).any() or dtype == torch.float32
    s, l, b, count = run(logits, boxes, sizes, 300, conf, nms)
    for i in range(B):
        want = expected_filtered(u[i], ub[i], conf, nms)
        c = int(count[i])
        assert c == len(want)
        assert torch.equal(l[i, :c], ul[i, want]) and torch.equal(b[i, :c], ub[i, want])
        assert torch.equal(s[i, :c], u[i, want])
    check_padding(s, l, b, count, 300)


@pytest.mark.parametrize("nq", [400, 900])          # 36 400 keys: resident form; 81 900: streamed form
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nms_at_k_1024(nq, dtype):
    """The largest LDS configuration (K = 1024: 16-word bitmask rows, ~156 KB) on both forms of the select."""
    B, C = 2, 91
    logits, _, sizes = rand_inputs(B, nq, C, dtype, seed=nq)
    g = torch.Generator().manual_seed(nq + 1)
    base = torch.rand(B, 60, 4, generator=g)
    pick = torch.randint(0, 60, (B, nq), generator=g)
    bb = torch.gather(base, 1, pick[..., None].expand(-1, -1, 4))
    boxes = torch.cat([bb[..., :2] * 0.8 + 0.1 + torch.randn(B, nq, 2, generator=g) * 0.02,
                       bb[..., 2:] * 0.3 + 0.03], -1).float().contiguous()
    u, ul, ub, _ = run(logits, boxes, sizes, 1024)
    for conf, nms in ((-1, 0.5), (0.3, 0.7)):
        s, l, b, count = run(logits, boxes, sizes, 1024, conf, nms)
        for i in range(B):
            want = expected_filtered(u[i], ub[i], conf, nms)
            c = int(count[i])
            assert 0 < c < 1024 and c == len(want)
            assert torch.equal(l[i, :c], ul[i, want]) and torch.equal(b[i, :c], ub[i, want])
            assert torch.equal(s[i, :c], u[i, want])
        check_padding(s, l, b, count, 1024)


def test_iou_threshold_is_compared_as_torchvision_does():
    """torchvision compares its fp32 IoU with the DOUBLE threshold.  Two boxes with IoU exactly 3/5 (fp32 0.60000002):
    3/5 > 0.6 in double, so the lower-ranked box is suppressed at threshold 0.6 (a compare against float32(0.6), which
    rounds up to 0.60000002, would keep it); at 0.6000001 it is kept."""
    logits = torch.tensor([[[2.0], [1.0]]])
    boxes = torch.tensor([[[2.0, 0.5, 4.0, 1.0], [3.0, 0.5, 4.0, 1.0]]])     # [0, 0, 4, 1] and [1, 0, 5, 1]
    sizes = torch.tensor([[1, 1]])
    s, l, b, count = run(logits, boxes, sizes, 2, -1, 0.6)
    assert count.tolist() == [1] and b[0, 0].tolist() == [0.0, 0.0, 4.0, 1.0]
    s, l, b, count = run(logits, boxes, sizes, 2, -1, 0.6000001)
    assert count.tolist() == [2]


def test_wrapper_refuses_16bit_boxes_on_the_device():
    logits, boxes, sizes = rand_inputs(2, 10, 5)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="pred_boxes must be float32"):
            detections_padded(logits.cuda(), boxes.to(dt).cuda(), sizes.cuda(), 10)
        with pytest.raises(RuntimeError, match="pred_boxes must be float32"):
            PostProcess(10)({"pred_logits": logits.cuda(), "pred_boxes": boxes.to(dt).cuda()}, sizes.cuda())


# ---- edges ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Nq,C,k", [(1, 900, 91, 1), (2, 10, 7, 70), (2, 900, 91, 1024), (16, 900, 91, 300),
                                      (2, 1, 91, 50), (2, 300, 1, 300), (1, 1, 1, 1), (2, 900, 366, 300),
                                      (1, 900, 366, 1024), (2, 450, 91, 300)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sizes_match_oracle(B, Nq, C, k, dtype):
    logits, boxes, sizes = rand_inputs(B, Nq, C, dtype, seed=B * 7 + Nq + C + k)
    s, l, b, count = run(logits, boxes, sizes, k)
    os_, ol, ob = oracle(logits, boxes, sizes, k)
    assert count.tolist() == [k] * B
    assert torch.equal(l, ol) and torch.equal(b, ob)
    assert ulps(s, os_).max() <= SCORE_ULPS


def test_streamed_rows_with_filters():
    """C = 366 at Nq = 900 (329 400 keys per image): the streamed form, with both filters."""
    logits, boxes, sizes = rand_inputs(2, 900, 366, seed=21)
    u, ul, ub, _ = run(logits, boxes, sizes, 300)
    s, l, b, count = run(logits, boxes, sizes, 300, 0.3, 0.5)
    for i in range(2):
        want = expected_filtered(u[i], ub[i], 0.3, 0.5)
        c = int(count[i])
        assert c == len(want) and torch.equal(l[i, :c], ul[i, want]) and torch.equal(b[i, :c], ub[i, want])


def test_logits_with_a_batch_stride_and_fp32_sizes():
    """A [:, pad:, :] query slice (what dn_post_process leaves) and fp32 target sizes."""
    full, boxes_full, sizes = rand_inputs(3, 1000, 91, seed=8)
    logits, boxes = full[:, 100:, :], boxes_full[:, 100:, :]
    out = detections_padded(full.cuda()[:, 100:, :], boxes_full.cuda()[:, 100:, :], sizes.float().cuda(), 300)
    s, l, b, count = [t.cpu() for t in out]
    os_, ol, ob = oracle(logits.contiguous(), boxes.contiguous(), sizes.float(), 300)
    assert torch.equal(l, ol) and torch.equal(b, ob) and ulps(s, os_).max() <= SCORE_ULPS


def test_infinities_and_signed_zeros():
    logits, boxes, sizes = rand_inputs(2, 100, 10, seed=9)
    logits[0, 5, 3] = float("inf")
    logits[0, 50, 1] = float("-inf")
    logits[1, :, :] = -5.0
    logits[1, 7, 2] = -0.0
    logits[1, 3, 4] = 0.0           # flat 34 < 72: +0.0 at the lower index wins the tie against -0.0
    logits[1, 90, 0] = -0.0
    logits[0, :, 0] = float("-inf")
    s, l, b, count = run(logits, boxes, sizes, 1000)
    os_, ol, ob = oracle(logits, boxes, sizes, 1000)
    assert torch.equal(l, ol) and torch.equal(b, ob) and ulps(s, os_).max() <= SCORE_ULPS
    assert s[0, 0] == 1.0 and l[0, 0] == 3
    assert l[1, :3].tolist() == [4, 2, 0] and s[1, 0] == 0.5
    assert (s[0, -100:] == 0).all()


def test_nan_logits_do_not_fault():
    logits, boxes, sizes = rand_inputs(2, 200, 91, seed=10)
    logits[0, ::3, ::2] = float("nan")
    logits[1].view(torch.int32)[::2, ::3] = -1          # the all-ones NaN pattern (the largest select key)
    s, l, b, count = run(logits, boxes, sizes, 300, 0.3, 0.5)
    assert ((l >= -1) & (l < 91)).all() and ((count >= 0) & (count <= 300)).all()
    s, l, b, count = run(logits, boxes, sizes, 300)
    assert ((l >= 0) & (l < 91)).all() and count.tolist() == [300, 300]


# ---- graph capture -------------------------------------------------------------------------------------------------

def test_graph_capture_replays_bit_for_bit():
    logits, boxes, sizes = rand_inputs(2, 900, 91, torch.bfloat16, seed=12)
    lg, bx, sz = logits.cuda(), boxes.cuda(), sizes.cuda()
    eager = [t.clone() for t in detections_padded(lg, bx, sz, 300, 0.3, 0.5)]
    torch.cuda.synchronize()
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        detections_padded(lg, bx, sz, 300, 0.3, 0.5)           # warm-up outside capture (library load, LDS attribute)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = detections_padded(lg, bx, sz, 300, 0.3, 0.5)
    torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    for t in out:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, out):
        assert torch.equal(e, r)


# ---- end to end ----------------------------------------------------------------------------------------------------

def test_postprocess_on_transformer_outputs_matches_torch_composite():
    from test_transformer_cpu import build_product_transformer, inputs
    d = np.load(os.path.join(G, "transformer_small.npz"))
    tr, _ = build_product_transformer(d)
    tr = tr.cuda()
    feats, masks, pos = inputs(d)
    with torch.no_grad():
        out_cls, out_box, _, _, _ = tr([f.cuda() for f in feats], [m.cuda() for m in masks], [p.cuda() for p in pos],
                                       None, None, None)
    logits, boxes = out_cls[-1], out_box[-1]
    B, Nq, C = logits.shape
    k = min(300, Nq * C)
    sizes = torch.tensor([[480, 640], [512, 400]][:B], dtype=torch.int64, device="cuda")
    res = PostProcess(k)({"pred_logits": logits, "pred_boxes": boxes}, sizes)
    # the reference's composite restated (torch.topk over sigmoid, gather, scale); order checked tie-free
    prob = logits.sigmoid()
    vals, idx = torch.topk(prob.view(B, -1), k, dim=1)
    qb = torch.div(idx, C, rounding_mode="trunc")
    cx, cy, w, h = boxes.unbind(-1)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    xyxy = torch.gather(xyxy, 1, qb.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    xyxy = xyxy * torch.stack([img_w, img_h, img_w, img_h], 1)[:, None, :]
    for i, r in enumerate(res):
        v = vals[i].cpu()
        assert ulps(r["scores"].cpu(), v).max() <= SCORE_ULPS
        distinct = torch.ones(k, dtype=torch.bool)
        distinct[1:] = v[1:] != v[:-1]
        distinct[:-1] &= v[:-1] != v[1:]
        assert torch.equal(r["labels"].cpu()[distinct], (idx[i] % C).cpu()[distinct])
        assert torch.allclose(r["boxes"].cpu()[distinct], xyxy[i].cpu()[distinct], rtol=0, atol=1e-4)
