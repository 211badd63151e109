"""GPU: a plain `bench.py` run -- the headline line with exactly `--steps` timed steps, and `--dump-outputs` writing what
the last step returned (`memory` and the four salience maps, float32, finite)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d
    levels = d["config"]["levels"]
    tokens = sum(h * w for h, w in levels)
    memory = np.load(tmp_path / "memory.npy")
    assert memory.dtype == np.float32 and memory.shape == (2, tokens, 256) and np.isfinite(memory).all()
    for i, (h, w) in enumerate(levels):
        s = np.load(tmp_path / ("salience_score_%d.npy" % i))
        assert s.dtype == np.float32 and s.shape == (2, 1, h, w) and np.isfinite(s).all()
    assert sorted(os.listdir(tmp_path)) == sorted(["memory.npy"] + ["salience_score_%d.npy" % i for i in range(len(levels))])
