"""The covariance-gated loop search with the candidates of all pending queries as one device batch (global search ->
refinement -> CS gate): Slam(batch_loop_search=True) and LocalFuser::detectLoopClosuresCovarianceGatedBatched() must build the
graph of the per-candidate methods called at the same moments, bit for bit.  The drive is the two-lap circle of
test_gpu_posegraph_cov_cpp.py, searched every 16 scans so that several queries are pending at a time."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

import randt_slam_amd as R
from randt_slam_amd import odometry, slam
from test_posegraph_cov import CovOracleBackend, _revisiting_drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "randt-slam_amd")
N_SCANS, DT, THR, DETECT_EVERY, OPTIMISE_EVERY = 230, 0.25, 0.5, 16, 40


def make_slam(backend, batched):
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    return slam.Slam(backend, mp, R.window_params(), R.default_matcher_params(gnc_steps=2), params=dict(submap_size_poses=40, submap_overlap=10),
                     loop_closure_weight=40.0, loop_search="covariance", max_data_association_mahalanobis_dist=THR, compute_dfs_loop_closure=True,
                     bnb_matcher_params=R.default_matcher_params(), batch_loop_search=batched)


def drive(s, scans):
    """Returns (poses per scan, node positions after every optimisation, seconds spent in detect_loop_closures)."""
    poses, after, spent = [], [], 0.0
    for i in range(len(scans)):
        s.process_scan(scans[i], i * DT)
        if i % DETECT_EVERY == DETECT_EVERY - 1:
            t0 = time.perf_counter()
            s.detect_loop_closures()
            spent += time.perf_counter() - t0
        if i % OPTIMISE_EVERY == OPTIMISE_EVERY - 1:
            s.optimize_pose_graph()
            after.append(s.node_positions().copy())
        poses.append(s.get_transform().copy())
    return np.array(poses), after, spent


def test_the_drive_has_batches_on_the_oracle(built):
    """What the GPU tests rest on, from the CPU oracle alone: searched every 16 scans the drive gives candidate batches of
    4, 4, 2 and 4 and six accepted edges.  (The oracle backend has no batch method: batch_loop_search falls back to the
    per-candidate loop, which is the same graph by definition.)"""
    s = make_slam(CovOracleBackend(), True)
    drive(s, _revisiting_drive(N_SCANS))
    batches = [n for n in s.loop_batches if n]
    print("batches", s.loop_batches, "log", s.loop_log)
    assert batches == [4, 4, 2, 4]
    assert sum(ok for _, _, _, ok in s.loop_log) == 6 and len(s.loop_log) == 14


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def python_runs(built):
    import torch

    scans = _revisiting_drive(N_SCANS)
    out = {}
    for batched in (False, True):
        ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
        b = odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params(), scan_slots=N_SCANS // 4 + 64, submap_slots=N_SCANS // 40 + 8)
        s = make_slam(b, batched)
        out[batched] = (s,) + drive(s, scans)
    return out


@pytest.mark.gpu
def test_batched_slam_builds_the_sequential_graph(python_runs):
    """T6: loop log (ids, CS values, flags), edges and their transforms, the node positions after every optimisation and the
    poses along the way, bit for bit."""
    (seq, seq_poses, seq_after, seq_s), (bat, bat_poses, bat_after, bat_s) = python_runs[False], python_runs[True]
    print("batches %s; %d candidates, %d accepted; loop search wall time: sequential %.1f ms, batched %.1f ms"
          % (bat.loop_batches, len(bat.loop_log), sum(ok for _, _, _, ok in bat.loop_log), 1e3 * seq_s, 1e3 * bat_s))
    assert max(bat.loop_batches) >= 3 and sum(ok for _, _, _, ok in bat.loop_log) >= 1
    assert seq.loop_batches == bat.loop_batches
    assert [(q, c, ok) for q, c, _, ok in seq.loop_log] == [(q, c, ok) for q, c, _, ok in bat.loop_log]
    assert same_bits([cs for _, _, cs, _ in seq.loop_log], [cs for _, _, cs, _ in bat.loop_log])
    assert [(a, b) for a, b, _, _ in seq.edges] == [(a, b) for a, b, _, _ in bat.edges]
    assert same_bits([e[2] for e in seq.edges], [e[2] for e in bat.edges])
    assert all(np.array_equal(a[3], b[3]) for a, b in zip(seq.edges, bat.edges))
    assert len(seq_after) == len(bat_after) == 5 and all(same_bits(a, b) for a, b in zip(seq_after, bat_after))
    assert same_bits(seq_poses, bat_poses)


def _build(tmp_path):
    exe = str(tmp_path / "loop_search_batched_drive")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "loop_search_batched_drive.cpp"),
        "-L", LIBDIR, "-lrandt_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe,
    ])
    return exe


def read_graph(path):
    nodes, loops, edges = [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == "node":
            nodes.append([float(v) for v in t[1:]])
        elif t[0] == "loop":
            loops.append((int(t[1]), int(t[2]), float(t[3]), int(t[4])))
        elif t[0] == "edge":
            edges.append((int(t[1]), int(t[2]), [float(v) for v in t[3:]]))
    return np.array(nodes), loops, edges


@pytest.mark.gpu
def test_cpp_batched_search_writes_the_sequential_graph(python_runs, tmp_path):
    """T7: the same drive through LocalFuser: detectLoopClosuresCovarianceGatedBatched() writes, byte for byte, the graph file
    detectLoopClosuresCovarianceGated() writes, and both are the Python harness's graph at the tolerances of
    test_gpu_posegraph_cov_cpp.py."""
    scans = np.ascontiguousarray(np.stack(_revisiting_drive(N_SCANS)), dtype=np.float32)
    path = tmp_path / "scans.bin"
    with open(path, "wb") as f:
        f.write(np.array([scans.shape[0], scans.shape[1]], dtype=np.int32).tobytes())
        f.write(scans.tobytes())
    exe = _build(tmp_path)
    graphs = {}
    for batched in (0, 1):
        graph = tmp_path / ("graph_%d.txt" % batched)
        r = subprocess.run([exe, str(path), str(graph), "40", "10", "%.17g" % THR, str(DETECT_EVERY), str(OPTIMISE_EVERY), str(batched)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert "covariance failed" not in r.stdout
        print(r.stdout.strip().splitlines()[-1])
        graphs[batched] = open(graph, "rb").read()
    assert graphs[0] == graphs[1] and len(graphs[0]) > 1000
    nodes, loops, edges = read_graph(tmp_path / "graph_1.txt")
    s = python_runs[True][0]
    assert len(nodes) == len(s.nodes) > 50 and sum(ok for _, _, _, ok in loops) >= 1
    assert [(q, c, ok) for q, c, _, ok in loops] == [(q, c, int(ok)) for q, c, _, ok in s.loop_log]
    assert np.allclose([cs for _, _, cs, _ in loops], [cs for _, _, cs, _ in s.loop_log], rtol=1e-9, atol=1e-12)
    assert [(a, b) for a, b, _ in edges] == [(a, b) for a, b, _, _ in s.edges]
    py_trans = np.array([[e[2][2], e[2][3], math.atan2(e[2][1], e[2][0])] for e in s.edges])
    assert np.abs(np.array([t for _, _, t in edges]) - py_trans).max() <= 1e-9
    assert np.abs(nodes - s.node_positions()).max() <= 1e-8
