"""
bench.py's own options: --steps is the number of timed steps, a plain run leaves the --full figures out, and
--dump-outputs writes the last timed step's results as float32 / float64 .npy files from seeded inputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "untuned", "basis_gather", "weak")


def _bench(*argv, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SVDQ_DIST_SINGLE", "SVDQ_DIST_BACKEND"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          env=env, timeout=timeout)


def test_bench_rejects_zero_steps():
    r = _bench("--steps", "0", timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr, (r.returncode, r.stderr[-500:])


def test_dump_row_sample_is_fixed():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.sample_rows(3, 10_000, 64)
    assert np.array_equal(a, bench.sample_rows(3, 10_000, 64)) and len(np.unique(a)) == 64
    assert np.all(np.diff(a) > 0) and a.min() >= 0 and a.max() < 10_000
    assert not np.array_equal(a, bench.sample_rows(4, 10_000, 64))
    assert np.array_equal(bench.sample_rows(0, 50, 64), np.arange(50))


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path):
    out = tmp_path / "dump"
    r = _bench("--model", "ViT-B-32", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert {"sigma.npy", "k.npy", "r.npy", "codes.npy", "scale.npy", "zero_point.npy", "c_high.npy", "basis_sample.npy",
            "mean_sample.npy", "sample_index.npy"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    k, r_ = files["k.npy"], files["r.npy"]
    assert len(k) == 152 and abs(float(k.mean()) - d["config"]["mean_rank_k"]) < 0.01
    U, idx = files["basis_sample.npy"], files["sample_index.npy"].astype(np.int64)
    assert U.shape == (len(idx), 8) and np.isfinite(U).all()
    cols = np.arange(8)[None, :]
    assert np.all(U[cols >= r_[idx[:, 0]][:, None]] == 0)          # zero beyond each parameter's r columns
    assert np.abs(U).sum(axis=0)[0] > 0
