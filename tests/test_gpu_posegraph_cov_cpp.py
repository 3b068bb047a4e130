"""-m gpu: the pose-graph covariances from C++ (tests/cpp/posegraph_cov_drive.cpp): GlobalFuser with
GlobalFuserParameters::compute_covariance fills Pose::cov* with the C ABI's numbers, and LocalFuser with
use_covariance_gated_loop_closure (the reference's loop search without Scan Context, local_fuser.cpp:351-412) produces the
graph of randt_slam_amd.slam.Slam(loop_search="covariance") on the same drive."""
import math
import os
import subprocess

import numpy as np
import pytest

import randt_slam_amd as R
from randt_slam_amd import host, odometry, slam, synth
import posegraph_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "randt-slam_amd")

pytestmark = pytest.mark.gpu


def _build(tmp_path):
    exe = str(tmp_path / "posegraph_cov_drive")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "posegraph_cov_drive.cpp"),
        "-L", LIBDIR, "-lrandt_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe,
    ])
    return exe


def test_global_fuser_fills_the_pose_covariances_with_the_abi_numbers(built, tmp_path):
    import torch

    _, x0, ia, ib, meas, sq = ref.make_graph(120, [(0, 119), (5, 110), (0, 60), (20, 100)], seed=0)
    file_meas = meas
    # an edge's angle goes through Sophus::SE2d(angle, ...) and trans.log()(2) on the C++ side: the same round trip for the ABI calls
    meas = meas.copy()
    meas[:, 2] = [math.atan2(math.sin(a), math.cos(a)) for a in meas[:, 2]]
    mui = 100                                                  # drops the late loop edges (0, 119) and (5, 110)
    path = tmp_path / "graph.txt"
    with open(path, "w") as f:
        f.write("%d %d\n" % (len(x0), len(ia)))
        for p in x0:
            f.write("%.17g %.17g %.17g\n" % tuple(p))
        for e in range(len(ia)):
            f.write("%d %d %.17g %.17g %.17g " % (ia[e], ib[e], file_meas[e][0], file_meas[e][1], file_meas[e][2]) + " ".join("%.17g" % v for v in sq[e].ravel()) + "\n")
    exe = _build(tmp_path)
    outs = {}
    for flag in (0, 1):
        out = tmp_path / ("nodes_%d.txt" % flag)
        r = subprocess.run([exe, "graph", str(path), str(out), str(mui), str(flag)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
        assert "covariance failed" not in r.stdout
        outs[flag] = np.loadtxt(out)
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    x1, _ = host.pose_graph_optimize(ctx, x0, ia, ib, meas, sq, mui)
    cov = host.pose_graph_covariance(ctx, x1, ia, ib, meas, sq, mui, None, -1)     # the LAST pose constant (global_fuser.cpp:68-69)
    for flag in (0, 1):
        assert np.array_equal(outs[flag][:, :3], x1)                                # the optimisation is the same with the flag on or off
    assert np.array_equal(outs[0][:, 3:], np.zeros((120, 16)))                      # flag off: always zero, as before
    got = outs[1]
    assert np.array_equal(got[:, 3:7], cov[:, :2, :2].reshape(-1, 4))               # cov_pos_pos, row-major 2x2
    assert np.array_equal(got[:, 7:9], cov[:, :2, 2])                               # cov_pos_rot
    assert np.array_equal(got[:, 9], cov[:, 2, 2])                                  # cov_rot_rot
    full = got[:, 10:].reshape(-1, 3, 3)                                            # Pose::cov assembled from them (:86-89)
    assert np.array_equal(full[:, :2, :], cov[:, :2, :]) and np.array_equal(full[:, 2, :2], cov[:, :2, 2]) and np.array_equal(full[:, 2, 2], cov[:, 2, 2])
    assert np.array_equal(full[-1], np.zeros((3, 3))) and np.abs(full[:-1]).reshape(119, -1).max(1).min() > 0


@pytest.mark.parametrize("dfs", [0, 1])
def test_cpp_covariance_gated_loop_search_matches_the_python_harness(built, tmp_path, dfs):
    import torch

    n_scans, per_lap, dt, thr = 230, 160, 0.25, 0.5
    world = synth.make_world()
    th = 2 * np.pi * np.arange(n_scans) / per_lap
    truth = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    scans = np.ascontiguousarray(np.stack([synth.make_scan(world, truth[i], 72000 + i) for i in range(n_scans)]), dtype=np.float32)
    path = tmp_path / "scans.bin"
    with open(path, "wb") as f:
        f.write(np.array([scans.shape[0], scans.shape[1]], dtype=np.int32).tobytes())
        f.write(scans.tobytes())
    exe = _build(tmp_path)
    out, graph = tmp_path / "poses.txt", tmp_path / "graph.txt"
    r = subprocess.run([exe, "drive", str(path), str(out), str(graph), "40", "10", str(dfs), "%.17g" % thr], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "covariance failed" not in r.stdout
    cpp_poses = np.loadtxt(out)
    nodes, loops, edges, covs = [], [], [], []
    for line in open(graph):
        t = line.split()
        if t[0] == "node":
            nodes.append([float(v) for v in t[1:]])
        elif t[0] == "loop":
            loops.append((int(t[1]), int(t[2]), float(t[3]), int(t[4])))
        elif t[0] == "edge":
            edges.append((int(t[1]), int(t[2]), [float(v) for v in t[3:]]))
        elif t[0] == "cov":
            covs.append([float(v) for v in t[2:]])
    nodes, covs = np.array(nodes), np.array(covs).reshape(-1, 3, 3)

    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    s = slam.Slam(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params(), scan_slots=n_scans // 4 + 64, submap_slots=n_scans // 40 + 8),
                  mp, R.window_params(), R.default_matcher_params(gnc_steps=2), params=dict(submap_size_poses=40, submap_overlap=10),
                  loop_closure_weight=40.0, loop_search="covariance", max_data_association_mahalanobis_dist=thr, compute_dfs_loop_closure=bool(dfs),
                  bnb_matcher_params=R.default_matcher_params())
    py_poses = []
    for i in range(n_scans):
        s.process_scan(scans[i], i * dt)
        s.detect_loop_closures()
        if i % 40 == 39:
            s.optimize_pose_graph()
        py_poses.append(s.get_transform().copy())
    py_poses = np.array(py_poses)
    print("dfs %d: %d candidates checked, %d accepted" % (dfs, len(s.loop_log), sum(ok for _, _, _, ok in s.loop_log)))
    assert s.n_covariance_failures == 0 and s.n_optimizations == 5
    assert len(nodes) == len(s.nodes) > 50
    assert [(q, c, ok) for q, c, _, ok in loops] == [(q, c, int(ok)) for q, c, _, ok in s.loop_log]          # same ids, same acceptances
    assert sum(ok for _, _, _, ok in loops) >= 1
    assert np.allclose([cs for _, _, cs, _ in loops], [cs for _, _, cs, _ in s.loop_log], rtol=1e-9, atol=1e-12)
    assert [(a, b) for a, b, _ in edges] == [(a, b) for a, b, _, _ in s.edges]
    py_trans = np.array([[e[2][2], e[2][3], math.atan2(e[2][1], e[2][0])] for e in s.edges])
    assert np.abs(np.array([t for _, _, t in edges]) - py_trans).max() <= 1e-9                                # transforms
    assert np.abs(nodes - s.node_positions()).max() <= 1e-8
    assert np.abs(covs - np.array(s.node_cov)).max() <= 1e-9 * np.abs(covs).max()
    assert np.abs(cpp_poses - py_poses).max() <= 1e-8, np.abs(cpp_poses - py_poses).max()
