"""CPU: bench.py's command line and its `--dump-outputs` writer -- float32 files, the byte budget, the same seeded sample
of an over-budget output on every run."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert _parse(monkeypatch, "--full").full
    for bad in (["--full", "--plain"], ["--steps", "0"], ["--dump-outputs", "d", "--in-flight", "2"]):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *bad)


def test_dump_outputs_writes_float32_whole_within_the_budget(tmp_path):
    mem = torch.randn(2, 300, 8).bfloat16()
    maps = [torch.rand(2, 1, 10, 12), torch.rand(2, 1, 5, 6)]
    bench.dump_outputs(str(tmp_path), {"memory": mem, "salience_score_0": maps[0], "salience_score_1": maps[1],
                                       "loss": torch.tensor([1.25], dtype=torch.float64)})
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["loss", "memory", "salience_score_0", "salience_score_1"]
    assert got["memory"].dtype == np.float32 and np.array_equal(got["memory"], mem.float().numpy())
    assert np.array_equal(got["salience_score_1"], maps[1].numpy())
    assert got["loss"].dtype == np.float64 and got["loss"][0] == 1.25


def test_dump_outputs_over_budget_is_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big, small = torch.randn(3, 1000), torch.randn(250)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big.clone(), "small": small.clone()})
    sizes = sum(np.load(tmp_path / "a" / f).nbytes for f in ("big.npy", "small.npy"))
    assert sizes <= 4000
    for f in ("big.npy", "small.npy"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.ndim == 1 and np.array_equal(a, b)
    # the sample is elements of the output, in flat-index order
    flat = big.flatten().numpy()
    pos = [int(np.flatnonzero(flat == v)[0]) for v in np.load(tmp_path / "a" / "big.npy")]
    assert pos == sorted(pos)
