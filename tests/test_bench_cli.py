"""bench.py's command line: a plain run prints the headline line and nothing that takes passes
of its own, --full adds those passes, --dump-outputs writes the last timed iterate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("phase_ms_per_iteration", "inner_ms_per_iteration", "host_enqueue_ms", "eager_body_ms",
             "cpu_baseline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_outputs_caps_the_size_with_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4096 + 2 * 8 * 100)   # 100 entries each
    big = np.arange(1000, dtype=np.float64) * 0.5
    small = np.array([1.0, 2.0, 3.0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (100,)
    assert np.array_equal(a, b)                                   # the same sample every time
    assert np.all(np.diff(a) > 0) and set(a) <= set(big)          # sorted, distinct entries of it
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    size = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert size <= bench.DUMP_LIMIT_BYTES


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_iterate(tmp_path):
    out = tmp_path / "dump"
    # 3 warm-up bodies, the body that re-captures the graph with the clock stamps and 60 timed
    # ones: the periodic restart (every 64 bodies) falls due right after the last timed body
    args = ("--config", "c1", "--steps", "60", "--warmup", "3")
    res = _bench(*args, "--dump-outputs", str(out))
    assert all(k in res for k in HEADLINE) and not any(k in res for k in FULL_ONLY)
    assert res["full"] is False and res["steps"] == 60 and res["warmup"] == 3
    assert res["value"] > 0 and abs(res["ms_per_step"] * res["value"] - 1e3) < 1e-6 * 1e3
    assert res["restarts"]["period"] == 1
    # c1: 2 clusters of one 4x4 block, 7 samples each, n_y = 4
    shapes = {"x": 14, "X": 32, "y": 4, "Y": 32, "stats": 9}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    arr = {n: np.load(out / (n + ".npy")) for n in shapes}
    for n, a in arr.items():
        assert a.dtype == np.float64 and a.shape == (shapes[n],) and np.all(np.isfinite(a)), n
    # an iterate, not the restart snapshot (X = 100 I, x = 0): X and Y are positive definite
    assert np.any(arr["x"] != 0.0) and not np.allclose(arr["X"].reshape(2, 4, 4), 100.0 * np.eye(4))
    for M in (arr["X"], arr["Y"]):
        for blk in M.reshape(2, 4, 4):
            assert np.allclose(blk, blk.T) and np.all(np.linalg.eigvalsh(blk) > 0)
    # the same arguments give the same outputs
    out2 = tmp_path / "dump2"
    _bench(*args, "--dump-outputs", str(out2))
    for n in shapes:
        assert np.array_equal(arr[n], np.load(out2 / (n + ".npy"))), n


@pytest.mark.gpu
def test_full_run_adds_the_other_passes():
    res = _bench("--config", "c1", "--steps", "4", "--warmup", "1", "--full", "--no-cpu")
    assert all(k in res for k in HEADLINE) and res["full"] is True
    assert all(k in res for k in FULL_ONLY if k != "cpu_baseline") and "cpu_baseline" not in res
    assert res["roofline"]["schur_ms_per_iteration"] > 0
    assert sum(res["phase_ms_per_iteration"].values()) > 0
