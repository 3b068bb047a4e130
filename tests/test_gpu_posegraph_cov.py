"""-m gpu: randt_pose_graph_covariance -- the selected inverse of the pose graph's information matrix on the device
(chain-segment recurrences + dense inverse of the Schur complement's factor) against the 60-digit fixture
tests/golden/posegraph_cov_01.npz and against dense float64 references (tests/posegraph_cov_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import randt_slam_amd as R
from randt_slam_amd import _capi, host
import posegraph_cov_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_cov_01.npz")


def _ctx():
    import torch

    return R.Context(0, torch.cuda.current_stream().cuda_stream)


def _case(g, name):
    return {k: g["%s__%s" % (name, k)] for k in ("x", "id_begin", "id_end", "meas", "sqrt_info", "anchor", "huber_a", "cov", "err_numpy", "cond")}


def test_fixture_cases_within_ten_times_the_float64_normal_equations(built):
    """Bar per case: block-relative error against the 60-digit blocks <= max(10 x err_numpy, 1e-12) -- both are float64
    normal-equation methods whose error scales with cond(H) eps; different elimination orders and serial recurrences
    on our side give the factor ten, the floor covers the cases where err_numpy is at rounding level."""
    g = np.load(GOLDEN)
    ctx = _ctx()
    failures = []
    for name in g["cases"]:
        c = _case(g, str(name))
        a = float(c["huber_a"])
        p = host.pg_params(use_robust_loss=1, loss_scale=a) if a > 0 else host.pg_params()
        cov = host.pose_graph_covariance(ctx, c["x"], c["id_begin"], c["id_end"], c["meas"], c["sqrt_info"], len(c["x"]), p, int(c["anchor"]))
        err = ref.block_rel_err(cov, c["cov"])
        bar = max(10.0 * float(c["err_numpy"]), 1e-12)
        print("fixture %-16s cond(H) %.2e err_numpy %.2e gpu err %.2e bar %.2e" % (name, float(c["cond"]), float(c["err_numpy"]), err, bar))
        assert np.array_equal(cov[int(c["anchor"])], np.zeros((3, 3)))
        if not err <= bar:
            failures.append((str(name), err, bar))
    assert not failures, failures


def _check_against_qr(ctx, x, ia, ib, meas, sq, mui, anchor, label, params=None, huber_a=0.0):
    """Bar: max(10 x the deviation of inv(J^T J) from the QR result, 1e-9).  Returns (gpu blocks, bar)."""
    n = len(x)
    J, var = ref.dense_jacobian(x, ia, ib, meas, sq, mui, anchor, huber_a)
    want = ref.cov_qr(n, J, var)
    dev = ref.block_rel_err(ref.cov_normal(n, J, var), want)
    bar = max(10.0 * dev, 1e-9)
    cov = host.pose_graph_covariance(ctx, x, ia, ib, meas, sq, mui, params, anchor)
    err = ref.block_rel_err(cov, want)
    print("structure %-28s n %4d anchor %4d: normal-vs-QR %.2e gpu-vs-QR %.2e bar %.2e" % (label, n, anchor, dev, err, bar))
    assert err <= bar, (label, err, bar)
    fixed = set(range(n)) - set(int(v) for v in var)
    for v in fixed:
        assert np.array_equal(cov[v], np.zeros((3, 3))), (label, v)
    return cov, bar


def test_structure_cases_against_a_qr_reference(built, monkeypatch):
    monkeypatch.delenv("RANDT_PG_SEGMENT", raising=False)
    ctx = _ctx()
    # no loop edges: pure chain recurrence, no Schur complement
    _, x, ia, ib, meas, sq = ref.make_graph(64, [], seed=2)
    _check_against_qr(ctx, x, ia, ib, meas, sq, 64, -1, "no loops")
    _check_against_qr(ctx, x, ia, ib, meas, sq, 64, 20, "no loops, interior anchor")
    # the same shape as a solver-independent known answer: on an open chain with diagonal sqrt-information the relative yaw
    # measurements are independent, yaw variance of pose k = |k - anchor| / 50^2.  Bar 1e-11 relative to the largest: at most
    # 39 steps of a 3x3 recurrence (some ten roundings each) times the conditioning of its blocks (xy against yaw, <= 1e3)
    _, x, ia, ib, meas, sq = ref.make_graph(40, [], seed=5)
    for anchor in (0, 39, 17):
        cov = host.pose_graph_covariance(ctx, x, ia, ib, meas, sq, 40, None, anchor)
        err = np.abs(cov[:, 2, 2] - np.abs(np.arange(40) - anchor) / 2500.0).max() / (39 / 2500.0)
        print("open chain, anchor %2d: yaw variance against |k - anchor| / 2500: %.2e relative" % (anchor, err))
        assert err <= 1e-11
    # a run longer than the 128-pose cut: separators that no loop closure made
    _, x, ia, ib, meas, sq = ref.make_graph(320, [(4, 290), (150, 20)], seed=12, radius=25.0)
    _check_against_qr(ctx, x, ia, ib, meas, sq, 320, -1, "320 poses, 128-cut")
    # nearly everything a separator
    _, x, ia, ib, meas, sq = ref.make_graph(90, [(0, 89), (3, 80), (10, 50)], seed=11)
    monkeypatch.setenv("RANDT_PG_SEGMENT", "4")
    _check_against_qr(ctx, x, ia, ib, meas, sq, 90, -1, "RANDT_PG_SEGMENT=4")
    monkeypatch.delenv("RANDT_PG_SEGMENT")
    # several loops meeting at pose 0; the anchor a separator, an interior, the first and the last pose
    _, x, ia, ib, meas, sq = ref.make_graph(70, [(0, 20), (0, 40), (0, 69), (5, 60)], seed=13)
    for anchor, what in ((40, "separator"), (33, "interior"), (0, "first"), (69, "last"), (-1, "last (-1)")):
        cov, _ = _check_against_qr(ctx, x, ia, ib, meas, sq, 70, anchor, "loops at pose 0, anchor " + what)
        assert np.array_equal(cov[69 if anchor == -1 else anchor], np.zeros((3, 3)))
    # adjacent separators, a reversed chain edge, duplicate odometry edges, full sqrt-information blocks, Huber
    _, x, ia, ib, meas, sq = ref.make_graph(40, [(0, 20), (7, 8), (12, 11), (30, 5), (29, 31), (30, 32)], seed=10)
    sq2 = sq + np.random.default_rng(8).normal(size=sq.shape) * 0.5
    _check_against_qr(ctx, x, ia, ib, meas, sq2, 40, -1, "full sqrt-information")
    meas2 = meas.copy()
    meas2[-1] += [2.0, -1.0, 0.3]
    _check_against_qr(ctx, x, ia, ib, meas2, sq, 40, 3, "Huber", host.pg_params(use_robust_loss=1, loss_scale=2.0), huber_a=2.0)
    # a pose that no used edge touches: zeros out
    x_pad = np.vstack([x, [[5.0, 5.0, 0.1]]])
    cov, _ = _check_against_qr(ctx, x_pad, ia, ib, meas, sq, 40, 0, "untouched pose")
    assert np.array_equal(cov[-1], np.zeros((3, 3))) and np.abs(cov[5]).max() > 0
    # late loop edges dropped by max_update_index (an edge is used iff id_begin + 1 == id_end || id_end <= max_update_index)
    _, x, ia, ib, meas, sq = ref.make_graph(50, [(0, 30), (2, 48)], seed=6)
    c_cut, bar = _check_against_qr(ctx, x, ia, ib, meas, sq, 40, 0, "max_update_index 40")
    c_all, _ = _check_against_qr(ctx, x, ia, ib, meas, sq, 49, 0, "max_update_index 49")
    c_ref = host.pose_graph_covariance(ctx, x, ia[:-1], ib[:-1], meas[:-1], sq[:-1], 49, None, 0)
    assert np.array_equal(c_cut, c_ref) and ref.block_rel_err(c_all, c_cut) > 1e-3


def test_elimination_order_invariance(built, monkeypatch):
    ctx = _ctx()
    _, x, ia, ib, meas, sq = ref.make_graph(200, [(0, 199), (20, 150), (60, 61 + 80)], seed=17, radius=20.0)
    covs = {}
    for seg in ("4", "16", None):
        if seg is None:
            monkeypatch.delenv("RANDT_PG_SEGMENT", raising=False)
        else:
            monkeypatch.setenv("RANDT_PG_SEGMENT", seg)
        covs[seg], bar = _check_against_qr(ctx, x, ia, ib, meas, sq, 200, -1, "segment cap %s" % seg)
    monkeypatch.delenv("RANDT_PG_SEGMENT", raising=False)
    for a, b in (("4", "16"), ("4", None), ("16", None)):
        d = ref.block_rel_err(covs[a], covs[b])
        print("order invariance %s vs %s: %.2e (bar %.2e)" % (a, b, d, bar))
        assert d <= bar


def _full_size_graph():
    n = 2200
    rng = np.random.default_rng(21)
    loops = [(int(a), int(a) + 1100 + int(o)) for a, o in zip(rng.integers(0, 1000, 60), rng.integers(-40, 40, 60))]
    _, x0, ia, ib, meas, sq = ref.make_graph(n, loops, seed=23, laps=2.0, radius=60.0)
    return n, loops, x0, ia, ib, meas, sq


def test_full_size_properties(built, monkeypatch):
    """The graph of test_hip_pose_graph_full_size_properties (2200 nodes, 60 loop closures): too large for a 60-digit
    inverse, so check what any exact marginal must satisfy."""
    monkeypatch.delenv("RANDT_PG_SEGMENT", raising=False)
    ctx = _ctx()
    n, loops, x0, ia, ib, meas, sq = _full_size_graph()
    x1, _ = host.pose_graph_optimize(ctx, x0, ia, ib, meas, sq, n)
    cov = host.pose_graph_covariance(ctx, x1, ia, ib, meas, sq, n, None, 0)
    assert np.array_equal(cov[0], np.zeros((3, 3)))
    asym = max(float(np.abs(c - c.T).max() / np.abs(c).max()) for c in cov[1:])
    min_eig = min(float(np.linalg.eigvalsh(0.5 * (c + c.T))[0]) for c in cov[1:])
    print("full size: worst relative asymmetry %.2e, smallest eigenvalue %.3e" % (asym, min_eig))
    assert asym <= 1e-12 and min_eig > 0
    # between the anchor and the nearest loop-closure pose the graph is a chain hanging off the anchor: the yaw variance
    # is (distance in edges) / 50^2 there (independent relative yaw measurements) and can only grow with the distance
    first, last = min(a for a, _ in loops), max(b for _, b in loops)
    cov_l = host.pose_graph_covariance(ctx, x1, ia, ib, meas, sq, n, None, -1)
    assert np.array_equal(cov_l[-1], np.zeros((3, 3))) and np.all(np.isfinite(cov_l))
    assert min(float(np.linalg.eigvalsh(0.5 * (c + c.T))[0]) for c in cov_l[:-1]) > 0
    stretches = [(what, yaw) for what, yaw in (("prefix, anchor 0", cov[:first + 1, 2, 2]), ("suffix, anchor last", cov_l[last:, 2, 2][::-1]))
                 if len(yaw) >= 3]
    assert stretches
    for what, yaw in stretches:
        known = np.abs(yaw - np.arange(len(yaw)) / 2500.0).max() / ((len(yaw) - 1) / 2500.0)
        print("full size: loop-free %s, %d poses, yaw variance %.6e .. %.6e, against k / 2500: %.2e relative" % (what, len(yaw), yaw[1], yaw[-1], known))
        assert np.all(np.diff(yaw) >= 0)
        assert known <= 1e-6   # cond(H) eps with cond(H) up to 1e9 at this size (weight-40 loops: 1e7 at 60 poses)


def test_rejected_inputs(built):
    ctx = _ctx()
    _, x, ia, ib, meas, sq = ref.make_graph(30, [(0, 29)], seed=3)
    for anchor in (30, -2, 1000):
        with pytest.raises(R.RandtError) as e:
            host.pose_graph_covariance(ctx, x, ia, ib, meas, sq, 30, None, anchor)
        assert e.value.status == _capi.ERR_INVALID
    bad = ib.copy()
    bad[3] = 77
    with pytest.raises(R.RandtError) as e:
        host.pose_graph_covariance(ctx, x, ia, bad, meas, sq, 100, None, 0)
    assert e.value.status == _capi.ERR_INVALID
    # a variable component that is not connected to the anchor (one chain edge and the loop edge gone): H is singular.
    # An ordinary rejected input: RANDT_ERR_INVALID, "rank deficient", h_cov untouched.
    keep = np.array([e_ for e_ in range(len(ia)) if e_ != 12 and e_ != len(ia) - 1])
    xa = np.ascontiguousarray(x)
    a32, b32 = np.ascontiguousarray(ia[keep]), np.ascontiguousarray(ib[keep])
    m, s = np.ascontiguousarray(meas[keep]), np.ascontiguousarray(sq[keep].reshape(-1, 9))
    out = np.full((30, 9), -7.25)
    p = host.pg_params()
    rc = ctx._lib.randt_pose_graph_covariance(ctx._h, 30, xa.ctypes.data, len(a32), a32.ctypes.data, b32.ctypes.data, m.ctypes.data,
                                              s.ctypes.data, 30, C.byref(p), 0, out.ctypes.data)
    assert rc == _capi.ERR_INVALID
    assert "rank deficient" in ctx._lib.randt_last_error(ctx._h).decode()
    assert np.all(out == -7.25)
    # the context is still good
    cov = host.pose_graph_covariance(ctx, x, ia, ib, meas, sq, 30, None, 0)
    assert np.all(np.isfinite(cov)) and np.abs(cov[7]).max() > 0
    # nothing to do: zeros
    assert np.array_equal(host.pose_graph_covariance(ctx, np.ones((3, 3)), [], [], np.zeros((0, 3)), np.zeros((0, 9)), 9), np.zeros((3, 3, 3)))


def test_the_optimiser_is_untouched_by_a_covariance_call(built):
    ctx = _ctx()
    _, x, ia, ib, meas, sq = ref.make_graph(300, [(4, 290), (150, 20)], seed=12, radius=25.0)
    x1, r1 = host.pose_graph_optimize(ctx, x, ia, ib, meas, sq, 300)
    host.pose_graph_covariance(ctx, x1, ia, ib, meas, sq, 300)
    x2, r2 = host.pose_graph_optimize(ctx, x, ia, ib, meas, sq, 300)
    assert np.array_equal(x1, x2) and r1 == r2
