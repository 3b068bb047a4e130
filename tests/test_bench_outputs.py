"""bench.py --dump-outputs without a GPU: float64 arrays, every row while they fit, a fixed seeded sample of rows above the cap."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import randt_slam_amd as R  # noqa: E402


def _records(n):
    rec = np.zeros(n, dtype=R.RESULT_DTYPE)
    rec["cost"] = np.arange(n) * 0.5
    rec["iterations"] = np.arange(n) % 7
    return rec


def test_small_batch_is_written_whole(tmp_path):
    pose = np.random.default_rng(1).standard_normal((512, 4))
    bench.write_outputs(str(tmp_path), pose, _records(512))
    assert not (tmp_path / "rows.npy").exists()
    assert np.array_equal(np.load(tmp_path / "pose.npy"), pose)
    it = np.load(tmp_path / "result_iterations.npy")
    assert it.dtype == np.float64 and np.array_equal(it, np.arange(512) % 7)
    assert not (tmp_path / "result_reserved.npy").exists()


def test_large_batch_is_a_fixed_sample_under_the_cap(tmp_path):
    n = bench.DUMP_BYTES_MAX // 8 // 4 + 1000
    pose = np.arange(n * 4, dtype=np.float64).reshape(n, 4)
    rec = _records(n)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), pose, rec)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sum(os.path.getsize(p) for p in a.iterdir()) <= bench.DUMP_BYTES_MAX + 4096
    rows = np.load(a / "rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(b / "rows.npy")) and len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(a / "pose.npy"), pose[rows])
    assert np.array_equal(np.load(a / "result_cost.npy"), rec["cost"][rows])
