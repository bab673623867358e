"""bench.py's plain run: one timed region of exactly --steps iterations, the headline fields, nothing of --full, and
--dump-outputs writing the same outputs from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_options_listed():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


def _plain(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "30", "--warmup", "5", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_times_exactly_its_steps_and_dumps_the_same_outputs(tmp_path):
    a, b = _plain(tmp_path / "a"), _plain(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 30 and d["warmup"] == 5 and d["warmup_effective"] == 1500 and d["n_gpus"] == 1
        assert d["reps"] == 1 and len(d["rep_values"]) == 1
        assert d["dtype"] == "f64" and d["higher_is_better"] is True and d["unit"].startswith("Gibbs iterations/s")
        assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) / d["value"] < 1e-9
        for k in ("roofline", "kernel_ms", "full_mode", "secondary", "cpu_baseline"):    # behind --full
            assert k not in d
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) == sorted(a["outputs"]["files"])
    assert files == ["E.npy", "P.npy", "ZsumG.npy", "ZsumK.npy", "metrics.npy"]
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.isfinite(x).all(), f
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), f
    met = np.load(tmp_path / "a" / "metrics.npy")
    assert met.shape == (9,)                                                    # the columns of a sweep without MH steps
    assert met[0] == 1 + a["warmup_effective"] + a["steps"]                     # the row of the last timed iteration (init is iteration 1)
    zk = np.load(tmp_path / "a" / "ZsumK.npy")
    assert zk.shape == (20, 10000) and zk.sum() == a["config"]["sum_M"]         # every count of that iteration allocated
