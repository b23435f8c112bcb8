"""bench.py --dump-outputs / --steps, CPU part: how the outputs are written and capped, and the argument check that runs
before anything touches torch or a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_npy_files(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(1)
    arrays = {"scores": rng.standard_normal(7), "distances": rng.standard_normal((7, 3)),
              "ref_embeddings": rng.standard_normal((3, 256)).astype(np.float32), "ints": np.arange(4)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["distances.npy", "ints.npy", "ref_embeddings.npy", "scores.npy"]
    for k, a in arrays.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == (np.float64 if a.dtype == np.float64 else np.float32), k
        assert np.array_equal(got, a), k


def test_dump_outputs_samples_the_same_rows_under_the_cap(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    big = np.arange(4000 * 64, dtype=np.float64).reshape(4000, 64)       # 2 MB
    small = np.arange(100, dtype=np.float64)
    limit = 1 << 20
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": small}, limit=limit)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and a.nbytes + np.load(tmp_path / "a" / "small.npy").nbytes <= limit
    rows = a[:, 0] / 64
    assert a.shape[1] == 64 and np.all(np.diff(rows) > 0) and np.array_equal(a, big[rows.astype(int)])   # whole rows, in order


def test_steps_below_one_is_an_argument_error():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stdout == "" and "--steps must be at least 1" in res.stderr
