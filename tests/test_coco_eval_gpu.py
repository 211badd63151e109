"""GPU: the COCO box evaluator's two HIP kernels (csrc/coco_eval.hip) against the loop restatement of
tests/coco_eval_cases.py.  Matched / ignored bits and counts exactly; precision, recall, scores and the 12 stats to
1e-12 (the same float64 operations; the slack covers a differently ordered mean).  The case builders assert that no
IoU lies within 1e-9 of a threshold, so exact bits are a fair demand."""
import os
import re

import numpy as np
import pytest
import torch

import coco_eval_cases as C
from salience_detr_amd import _hip, coco_eval as E, graph_guard
from salience_detr_amd.coco_eval import CocoBoxEvaluator

pytestmark = pytest.mark.gpu
TOL = 1e-12
KNOWN = {
    "A": [1, 1, 1, 1, -1, -1, 1, 1, 1, 1, -1, -1],
    "B": [0.5, 0.5, 0.5, None, None, None, 0, 1, 1, None, None, None],
    "C": [0.6, 1, 1, -1, -1, 0.6, None, None, 0.6, None, None, None],
    "D": [-1] * 12,
    "E": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],
}


def run_evaluator(category_ids, images, batches=None):
    ev = CocoBoxEvaluator(category_ids, device="cuda")
    for batch in (batches or [list(range(len(images)))]):
        ev.update(*C.as_update_args([images[i] for i in batch], "cuda"))
    ev.accumulate()
    ev.summarize(verbose=False)
    return ev


def assert_equals_restatement(ev, want):
    det, gt = ev._records()
    assert det.is_cuda and C.record_bits(det) == want["bits"]
    assert C.record_npig(gt) == want["npig"]
    for name in ("precision", "recall", "scores"):
        assert ev.eval[name].dtype == torch.float64 and tuple(ev.eval[name].shape) == want[name].shape
        assert np.abs(ev.eval[name].numpy() - want[name]).max() <= TOL, name
    assert np.abs(ev.stats.numpy() - want["stats"]).max() <= TOL


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    category_ids, images = C.known_cases()[name]
    ev = run_evaluator(category_ids, images)
    for value, known in zip(ev.stats.tolist(), KNOWN[name]):
        assert known is None or abs(value - known) <= TOL, (name, ev.stats)
    assert_equals_restatement(ev, C.restate(category_ids, images))


@pytest.fixture(scope="module")
def scene():
    category_ids, images = C.random_scene()
    return category_ids, images, C.restate(category_ids, images)


def test_random_scene_and_batch_order(scene):
    category_ids, images, want = scene
    a = run_evaluator(category_ids, images)
    assert_equals_restatement(a, want)
    b = run_evaluator(category_ids, images, batches=[[3], [1, 0, 2]])
    assert_equals_restatement(b, want)
    for name in ("precision", "recall", "scores"):
        assert torch.equal(a.eval[name], b.eval[name]), name


def test_cap_at_100(scene):
    category_ids, images = C.cap_scene()
    assert_equals_restatement(run_evaluator(category_ids, images), C.restate(category_ids, images))


def test_ground_truths_above_capacity_raise():
    cap = _hip.lib().sdetr_coco_eval_gt_capacity()
    assert cap == E.GT_CAPACITY
    gts = [(1, [i, 0, i + 10, 10]) for i in range(cap + 1)]
    ev = CocoBoxEvaluator([1], device="cuda")
    with pytest.raises(RuntimeError, match="capacity"):
        ev.update(*C.as_update_args([C.image(1, [(0.5, 1, [0, 0, 10, 10])], gts)], "cuda"))


def test_accumulate_carries_the_scan_over_chunks():
    """2 chunks + 3 records in ONE category (synthetic bits, ranks up to 29 so that maxDet 1 and 10 filter, tied scores),
    an empty second category."""
    header = open(_hip.HEADER_PATH).read()
    chunk = int(re.search(r"#define\s+SDETR_COCO_ACC_CHUNK\s+(\d+)", header).group(1))
    assert _hip.lib().sdetr_coco_eval_chunk_records() == chunk
    n = 2 * chunk + 3
    rng = np.random.default_rng(5)
    scores = np.sort(rng.integers(1, 400, n).astype(np.float32) / 512)[::-1].astype(np.float64)
    ranks = rng.integers(0, 30, n)
    ranks[:4] = [12, 0, 3, 0]
    matched = rng.integers(0, 1 << 40, n, dtype=np.int64) & rng.integers(0, 1 << 40, n, dtype=np.int64)
    ignored = rng.integers(0, 1 << 40, n, dtype=np.int64) & rng.integers(0, 1 << 40, n, dtype=np.int64) \
        & rng.integers(0, 1 << 40, n, dtype=np.int64)
    npig = [700, 61, 0, 2500]
    rows = torch.tensor(np.stack([np.arange(n), ranks.astype(np.int64) << 32, scores.view(np.int64), matched, ignored], 1))
    first = torch.tensor([0, n, n])
    counts = torch.tensor([npig, [0, 0, 0, 0]])
    thresholds = torch.from_numpy(C.REC_THRS)
    precision, recall, out_scores = E.hip_accumulate(rows.cuda(), first.cuda(), counts.cuda(), 2, thresholds.cuda())
    want_p, want_r, want_s = C.accumulate_rows(ranks.tolist(), scores.tolist(), matched.tolist(), ignored.tolist(), npig)
    assert np.abs(precision[:, :, 0].cpu().numpy() - want_p).max() <= TOL
    assert np.abs(recall[:, 0].cpu().numpy() - want_r).max() <= TOL
    assert np.abs(out_scores[:, :, 0].cpu().numpy() - want_s).max() <= TOL
    assert (precision[:, :, 1] == -1).all() and (recall[:, 1] == -1).all() and (out_scores[:, :, 1] == -1).all()
    assert (want_p[:, :, 2] == -1).all() and want_r[0, 0, 2] > 0
    # the torch composite on the same records
    comp = E._composite_accumulate(rows, first, counts, 2, thresholds)
    for got, ref in zip((precision, recall, out_scores), comp):
        assert np.abs(got.cpu().numpy() - ref.numpy()).max() <= TOL


def test_update_replays_bit_for_bit_under_graph_capture(scene):
    category_ids, images, _ = scene
    ev = CocoBoxEvaluator(category_ids, device="cuda")
    detections, targets = C.as_update_args(images, "cuda")
    lut, thr, _ = ev._constants()
    args = tuple(t.contiguous() for t in E.pad_detections(detections)) + E.pad_targets(targets, torch.device("cuda"))
    eager = [t.clone() for t in E.hip_update(*args, lut, 3, thr)]
    torch.cuda.synchronize()
    out = tuple(torch.empty_like(t) for t in eager)
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            E.hip_update(*args, lut, 3, thr, out=out)
    torch.cuda.current_stream().wait_stream(stream)
    assert graph_guard.memset_nodes(graph) == 0
    replays = []
    for fill in (7, -3):
        for t in out:
            t.fill_(fill)                                   # fresh buffers: nothing of the last run is left
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in out])
    for e, a, b in zip(eager, *replays):
        assert torch.equal(a, b) and torch.equal(e, a)
    assert int(eager[2][0]) == sum(1 for key in C.restate(category_ids, images)["bits"])


def test_detections_padded_route_equals_list_of_dicts():
    from salience_detr_amd.post_process import detections_padded
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(2, 40, 9, generator=g) * 2).cuda()
    centre, size = torch.rand(2, 40, 2, generator=g) * 0.6 + 0.2, torch.rand(2, 40, 2, generator=g) * 0.3 + 0.05
    boxes = torch.cat([centre, size], -1).cuda()
    sizes = torch.tensor([[200, 300], [240, 180]]).cuda()
    padded = detections_padded(logits, boxes, sizes, 25, confidence_score=0.3)
    counts = padded[3].tolist()
    assert 0 < min(counts) and max(counts) <= 25
    dicts = [{"scores": padded[0][i, :c], "labels": padded[1][i, :c], "boxes": padded[2][i, :c]} for i, c in enumerate(counts)]
    rng = np.random.default_rng(9)
    images = []
    for i in range(2):
        src = padded[2][i, :counts[i]].cpu().numpy().round()
        lab = padded[1][i, :counts[i]].cpu().numpy()
        # every other detection gives a ground truth: its box rounded to the grid (each edge moves at most half a pixel
        # on boxes at least 9 wide: IoU > 0.5), or a random box; some are crowds
        gts = [(int(lab[j]), [float(v) for v in src[j]] if j % 4 == 0 else C._random_box(rng), 1 if j % 5 == 4 else 0)
               for j in range(0, counts[i], 2)]
        images.append(C.image(10 - i, [], gts))
    _, targets = C.as_update_args(images, "cuda")
    category_ids = [0, 1, 2, 4, 5, 7, 8]                        # labels 3 and 6 are dropped
    a, b = CocoBoxEvaluator(category_ids), CocoBoxEvaluator(category_ids)
    a.update(padded, targets)
    b.update(dicts, targets)
    assert a.device.type == "cuda"
    a.summarize(verbose=False)
    b.summarize(verbose=False)
    assert torch.equal(a._records()[0], b._records()[0]) and torch.equal(a._records()[1], b._records()[1])
    for name in ("precision", "recall", "scores"):
        assert torch.equal(a.eval[name], b.eval[name])
    assert (a.stats[:2] > 0).all()                              # mAP and AP50: the rounded copies match at 0.5
    # and against the restatement, from the same detections
    for i in range(2):
        images[i]["det_scores"] = padded[0][i, :counts[i]].float().cpu().numpy()
        images[i]["det_labels"] = padded[1][i, :counts[i]].cpu().numpy()
        images[i]["det_boxes"] = padded[2][i, :counts[i]].cpu().numpy()
    assert C.clear_of_thresholds(images)
    assert_equals_restatement(a, C.restate(category_ids, images))
