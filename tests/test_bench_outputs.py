"""`bench.py --gpus 1` without `--full`: the lean headline line, and `--dump-outputs DIR` -- the last timed step's results
written as .npy, identical from run to run on the same arguments (seeded corpus and queries)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--passages", "40000", "--doclen", "64", "--batch", "128", "--sub-batch", "64", "--query-batches", "2"]


def _bench(extra, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + extra + ["--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = _bench(["--steps", "3", "--warmup", "1"], tmp_path / "a")
    assert rec["metric"] == "queries/sec" and rec["unit"] == "queries/sec" and rec["higher_is_better"] is True
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["dtype"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 128 / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["recall_at_5"] >= 0.95, rec["recall_at_5"]
    for key in ("roofline", "cpu_baseline", "sub_results", "latency", "stage_ms_per_step"):   # --full only
        assert key not in rec, key
    p, s, c = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("pids", "scores", "counts"))
    assert p.dtype == np.float64 and s.dtype == np.float32 and c.dtype == np.float64
    assert p.shape == s.shape == (128, 100) and c.shape == (128,)
    n = c.astype(np.int64)
    assert ((n >= 1) & (n <= 100)).all()
    valid = np.arange(100)[None, :] < n[:, None]
    assert (p[valid] >= 0).all() and (p[valid] < 40000).all() and (p[~valid] == -1).all() and (s[~valid] == 0).all()
    assert (np.diff(np.where(valid, s, -np.inf), axis=1)[valid[:, 1:]] <= 0).all()   # scores descending within each list
    # another run with the same arguments (more steps: the last one lands on the same query batch) returns the same arrays
    _bench(["--steps", "5", "--warmup", "2"], tmp_path / "b")
    for name in ("pids", "scores", "counts"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
