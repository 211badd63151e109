"""CPU: the COCO box evaluator's torch composite against the loop restatement (tests/coco_eval_cases.py) and against
answers known in advance.  The same float64 operations on both sides, so arrays agree to 1e-12 (a differently ordered
mean is all the slack covers) and the matched / ignored bits exactly."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import coco_eval_cases as C
from salience_detr_amd.coco_eval import METRIC_NAMES, CocoBoxEvaluator, evaluate

TOL = 1e-12


def run_evaluator(category_ids, images, batches=None, device="cpu"):
    ev = CocoBoxEvaluator(category_ids, device=device)
    for batch in (batches or [list(range(len(images)))]):
        ev.update(*C.as_update_args([images[i] for i in batch], device))
    ev.accumulate()
    ev.summarize(verbose=False)
    return ev


def assert_equals_restatement(ev, want):
    det, gt = ev._records()
    assert C.record_bits(det) == want["bits"]
    assert C.record_npig(gt) == want["npig"]
    for name in ("precision", "recall", "scores"):
        assert ev.eval[name].dtype == torch.float64 and tuple(ev.eval[name].shape) == want[name].shape
        assert np.abs(ev.eval[name].numpy() - want[name]).max() <= TOL, name
    assert np.abs(ev.stats.numpy() - want["stats"]).max() <= TOL
    assert ev.eval["counts"] == [10, 101, want["recall"].shape[1], 4, 3]


KNOWN = {
    "A": [1, 1, 1, 1, -1, -1, 1, 1, 1, 1, -1, -1],
    "B": [0.5, 0.5, 0.5, None, None, None, 0, 1, 1, None, None, None],
    "C": [0.6, 1, 1, -1, -1, 0.6, None, None, 0.6, None, None, None],
    "D": [-1] * 12,
    "E": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],          # area exactly 1024: small AND medium, not large
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    category_ids, images = C.known_cases()[name]
    want = C.restate(category_ids, images)
    ev = run_evaluator(category_ids, images)
    for got in (want["stats"], ev.stats.numpy()):          # the restatement first: if it disagrees, it is wrong
        for value, known in zip(got, KNOWN[name]):
            assert known is None or abs(value - known) <= TOL, (name, got)
    assert_equals_restatement(ev, want)


@pytest.fixture(scope="module")
def scene():
    category_ids, images = C.random_scene()
    return category_ids, images, C.restate(category_ids, images)


def test_random_scene_equals_restatement(scene):
    category_ids, images, want = scene
    assert sorted(len(im["det_labels"]) for im in images)[0] == 0 and sorted(len(im["gt_labels"]) for im in images)[0] == 0
    assert any(7 in im["det_labels"] for im in images) and any(im["gt_crowd"].any() for im in images)
    ev = run_evaluator(category_ids, images)
    assert_equals_restatement(ev, want)
    assert (want["stats"] > -1).all() and 0 < want["stats"][0] < 1          # the case is not degenerate


def test_cap_at_100_and_ranks(scene):
    category_ids, images = C.cap_scene()
    want = C.restate(category_ids, images)
    ev = run_evaluator(category_ids, images)
    assert_equals_restatement(ev, want)
    det, _ = ev._records()
    ranks = sorted(rank for (image_id, k, rank) in C.record_bits(det) if image_id == 8 and k == 1)
    assert ranks == list(range(100))
    assert not np.array_equal(want["recall"][:, 1, 0, 0], want["recall"][:, 1, 0, 2])     # maxDet 1 differs from 100


def test_batch_split_and_order_do_not_matter(scene):
    category_ids, images, want = scene
    a = run_evaluator(category_ids, images, batches=[[0, 1], [2, 3]])
    b = run_evaluator(category_ids, images, batches=[[3], [1, 0, 2]])
    for name in ("precision", "recall", "scores"):
        assert torch.equal(a.eval[name], b.eval[name]), name
    assert torch.equal(a.stats, b.stats)
    assert_equals_restatement(a, want)


def test_update_refuses_an_image_seen_twice(scene):
    import salience_detr_amd
    assert salience_detr_amd.CocoBoxEvaluator is CocoBoxEvaluator and salience_detr_amd.evaluate is evaluate
    category_ids, images, _ = scene
    ev = CocoBoxEvaluator(category_ids)
    ev.update(*C.as_update_args(images[:2]))
    with pytest.raises(RuntimeError, match="seen twice"):
        ev.update(*C.as_update_args(images[1:3]))
    with pytest.raises(RuntimeError, match="seen twice"):
        CocoBoxEvaluator(category_ids).update(*C.as_update_args([images[0], images[0]]))


def test_padded_tuple_equals_list_of_dicts(scene):
    """The 4-tuple of ``detections_padded`` (fixed shape, count, padding label -1) and ``PostProcess``'s list of dicts."""
    from salience_detr_amd.coco_eval import pad_detections
    category_ids, images, want = scene
    detections, targets = C.as_update_args(images)
    ev = CocoBoxEvaluator(category_ids)
    ev.update(pad_detections(detections), targets)
    ev.summarize(verbose=False)
    assert_equals_restatement(ev, want)


def test_summary_lines_table_and_evaluate(scene, capsys):
    category_ids, images, want = scene
    ev = run_evaluator(category_ids, images)
    ev.summarize()
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % want["stats"][0]
    assert lines[1].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = ")
    assert lines[6].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = ")
    assert lines[11].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ")
    table = ev.per_category_table(["two", "five", "eleven"])
    assert table[0] == ["class", "imgs", "gts", "dets", "recall", "ap"] and len(table) == 5
    cats = sorted(category_ids)
    for k, row in enumerate(table[1:4]):
        assert row[0] == ["two", "five", "eleven"][k]
        assert row[1] == sum(1 for im in images if cats[k] in im["gt_labels"])
        assert row[2] == sum(int((im["gt_labels"] == cats[k]).sum()) for im in images)
        assert row[3] == sum(int((im["det_labels"] == cats[k]).sum()) for im in images)
        assert row[4] == "%.3f" % want["recall"][0, k, 0, 2] and row[5] == "%.3f" % want["precision"][0, :, k, 0, 2].mean()
    assert table[4][0] == "mean results" and table[4][5] == "%.3f" % want["stats"][1]

    class Model(torch.nn.Module):
        def forward(self, batch):
            return [detections[i] for i in batch]
    detections, targets = C.as_update_args(images)
    model = Model().train()
    ev2, metrics = evaluate(model, [([0, 1], targets[:2]), ([2, 3], targets[2:])], category_ids, verbose=False)
    assert not model.training and tuple(metrics) == METRIC_NAMES
    assert np.abs(np.array(list(metrics.values())) - want["stats"]).max() <= TOL
    assert torch.equal(ev2.eval["precision"], ev.eval["precision"])


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        category_ids, images = C.random_scene()
        ev = CocoBoxEvaluator(category_ids)
        mine = [images[0], images[2]] if rank == 0 else [images[3], images[1]]
        ev.update(*C.as_update_args(mine))
        ev.synchronize_between_processes()
        ev.accumulate()
        ev.summarize(verbose=False)
        torch.save({"eval": ev.eval, "stats": ev.stats}, os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one_process(tmp_path, scene):
    category_ids, images, want = scene
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single = run_evaluator(category_ids, images)
    for rank in range(2):
        got = torch.load(os.path.join(tmp_path, f"r{rank}.pt"))
        for name in ("precision", "recall", "scores"):
            assert torch.equal(got["eval"][name], single.eval[name]), (rank, name)
        assert torch.equal(got["stats"], single.stats)
    assert np.abs(single.stats.numpy() - want["stats"]).max() <= TOL
