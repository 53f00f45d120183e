"""bench.py's plain run and --dump-outputs: the plain line holds the headline fields and nothing that --full adds, and the dump
holds what the last timed step returned (CPU: the writer and its size cap; GPU: a small end-to-end run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Fit:
    def __init__(self, p, nl, seed=0):
        rng = np.random.default_rng(seed)
        self.lambda_ = np.geomspace(1.0, 1e-2, nl)
        self.niter = rng.integers(1, 200, nl).astype(np.int32)
        self.beta_dense = np.asfortranarray(rng.standard_normal((p + 1, nl)).astype(np.float32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    fit = _Fit(50, 7)
    bench.dump_outputs(fit, str(tmp_path / "out"))
    got = _load(tmp_path / "out")
    assert sorted(got) == ["beta", "lambda", "niter"]
    assert got["lambda"].dtype == np.float64 and got["niter"].dtype == np.float64 and got["beta"].dtype == np.float32
    assert np.array_equal(got["lambda"], fit.lambda_) and np.array_equal(got["niter"], fit.niter.astype(np.float64))
    assert np.array_equal(got["beta"], fit.beta_dense)


def test_dump_outputs_samples_rows_under_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    fit = _Fit(20_000, 10)
    for d in ("a", "b"):
        bench.dump_outputs(fit, str(tmp_path / d))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 200_000
    rows = a["beta_rows"].astype(np.int64)
    assert a["beta_rows"].dtype == np.float64 and 0 < len(rows) < fit.beta_dense.shape[0] and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["beta"], fit.beta_dense[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)                 # the sample is fixed: two dumps compare row for row


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "24000", "--p", "2304",
           "--m", "100", "--nlambda", "12", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"cpu_baseline", "configs", "consensus", "setup_s"} & set(line), sorted(line)
    got = _load(out)
    assert got["lambda"].shape == (12,) and got["niter"].shape == (12,) and got["beta"].shape == (2305, 12)
    assert np.all(got["niter"] >= 1) and np.all(np.isfinite(got["beta"]))
