"""-m gpu: place recognition for scans outside the database through the C++ facade (tests/cpp/sc_query_drive.cpp):
SCManager::queryLoopClosure and SCManager::appendNode give the ids, yaws and candidate lists of the C entries on the same scans."""
import os
import subprocess

import numpy as np
import pytest

from randt_slam_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "randt-slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "sc_query_drive")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sc_query_drive.cpp"),
        "-L", LIBDIR, "-lrandt_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe,
    ])
    return exe


def test_cpp_query_and_restore_equal_the_c_entries(built, tmp_path):
    world = synth.make_world()
    n_db, n_q = 16, 4
    traj = synth.make_trajectory(3100, n_db, step=0.6)
    # the queries: held-out scans next to database poses (their own noise), in another heading
    q_poses = np.stack([traj[i] + np.array([0.15, -0.1, 0.6 + 0.3 * k]) for k, i in enumerate((2, 6, 9, 13))])
    poses = np.concatenate([traj, q_poses])
    scans = np.stack([synth.make_scan(world, poses[i], 8100 + i) for i in range(n_db + n_q)]).astype(np.float32)
    pos = poses[:, :2].astype(np.float64)
    dist = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(pos[:n_db], axis=0).T)), 40.0 + np.arange(n_q)])
    path = tmp_path / "scans.bin"
    with open(path, "wb") as f:
        f.write(np.array([n_db, n_q, scans.shape[1]], dtype=np.int32).tobytes())
        f.write(scans.tobytes())
        f.write(pos.tobytes())
        f.write(dist.tobytes())
    r = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERENT" not in r.stdout and r.stdout.count(": equal") == 9, r.stdout
