#!/usr/bin/env python3
"""Generator of tests/golden/posegraph_cov_01.npz: marginal covariances of small pose graphs at 60 digits.

Our own numpy + mpmath; nothing of the reference or of the oracle is involved.  Per case: a graph from the recipe of
tests/test_posegraph.py::make_graph (copied below), the dense Jacobian J of the used edges from the written-out edge
Jacobians of PoseGraph2dErrorTerm (sqrt-information applied, sqrt(rho') of the Huber loss when the case is robust), the
anchor's columns deleted, (J^T J)^-1 at 60 digits.  Stored: the inputs, the anchor, the 3x3 diagonal blocks rounded to
double (zeros for the anchor) and err_numpy = the block-relative error (max-abs of a block's difference over the max-abs
of the true block, worst block) of plain float64 np.linalg.inv(J.T @ J) against the 60-digit result -- the yardstick the
GPU test scales its bar with.

    python tests/golden/make_posegraph_cov.py            # all cases, a few minutes (one process per case)
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ODOM_SQI = np.diag([10.0, 10.0, 50.0])   # local_fuser.cpp:203-205


def rel(a, b):
    c, s = np.cos(a[2]), np.sin(a[2])
    d = b[:2] - a[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], (b[2] - a[2] + np.pi) % (2 * np.pi) - np.pi])


def compose(a, m):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * m[0] - s * m[1], a[1] + s * m[0] + c * m[1], a[2] + m[2]])


def make_graph(n, loops, seed=0, noise=(0.02, 0.02, 0.005), loop_weight=40.0, laps=1.0, radius=10.0):
    """Circular drive with noisy odometry edges (dead-reckoned initial guess) and the given loop-closure pairs."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi * laps, n, endpoint=False)
    truth = np.stack([radius * np.cos(th), radius * np.sin(th), th + np.pi / 2], 1)
    ia, ib, meas, sq = [], [], [], []
    for i in range(n - 1):
        ia.append(i)
        ib.append(i + 1)
        meas.append(rel(truth[i], truth[i + 1]) + rng.normal(size=3) * noise)
        sq.append(ODOM_SQI)
    n_odom = len(ia)
    for a, b in loops:
        ia.append(a)
        ib.append(b)
        meas.append(rel(truth[a], truth[b]) + rng.normal(size=3) * np.array(noise) * 0.5)
        sq.append(np.eye(3) * loop_weight)
    x0 = [truth[0].copy()]
    for i in range(n_odom):
        x0.append(compose(x0[-1], meas[i]))
    return truth, np.array(x0), np.array(ia, np.int32), np.array(ib, np.int32), np.array(meas), np.array(sq)


# name, poses, loops, loop weight, anchor, robust (Huber a, or 0), seed
CASES = [
    ("w40_last", 60, [(0, 59), (10, 45)], 40.0, 59, 0.0, 41),
    ("w4e4_first", 60, [(0, 59), (10, 45)], 4.0e4, 0, 0.0, 42),
    ("w40_interior", 50, [(0, 49), (5, 40), (12, 30)], 40.0, 25, 0.0, 43),
    ("w4e4_loop_pose", 48, [(0, 47), (3, 40), (8, 30), (15, 25)], 4.0e4, 30, 0.0, 44),
    ("w40_five_loops", 40, [(0, 39), (2, 35), (6, 30), (10, 25), (0, 20)], 40.0, 39, 0.0, 45),
    ("huber_outlier", 56, [(0, 55), (10, 45)], 40.0, 55, 2.0, 46),
]


def edge_jacobians(F, x, ia, ib, meas, sq, huber_a):
    """Rows of J per edge: (3x3 d r / d pose_a, 3x3 d r / d pose_b) with number type F (float or mpmath.mpf)."""
    if F is float:
        import math as M

        sqrt, sin, cos, pi, floor = M.sqrt, M.sin, M.cos, M.pi, M.floor
    else:
        import mpmath as M

        sqrt, sin, cos, pi, floor = M.sqrt, M.sin, M.cos, M.pi, M.floor
    out = []
    for e in range(len(ia)):
        pa, pb = [F(v) for v in x[ia[e]]], [F(v) for v in x[ib[e]]]
        ms = [F(v) for v in meas[e]]
        S = [[F(sq[e][i][j]) for j in range(3)] for i in range(3)]
        s, c = sin(pa[2]), cos(pa[2])
        dx, dy = pb[0] - pa[0], pb[1] - pa[1]
        a = (pb[2] - pa[2]) - ms[2]
        ev = [(c * dx + s * dy) - ms[0], (-s * dx + c * dy) - ms[1], a - 2 * pi * floor((a + pi) / (2 * pi))]
        A = [[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [F(0), F(0), F(-1)]]
        B = [[c, s, F(0)], [-s, c, F(0)], [F(0), F(0), F(1)]]
        r = [sum(S[i][k] * ev[k] for k in range(3)) for i in range(3)]
        w = F(1)
        if huber_a > 0:   # ceres::HuberLoss(a): rho' = a / sqrt(s) beyond s = a^2; Covariance applies the loss by default
            sn = sum(v * v for v in r)
            if sn > F(huber_a) ** 2:
                w = sqrt(F(huber_a) / sqrt(sn))
        Ja = [[w * sum(S[i][k] * A[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        Jb = [[w * sum(S[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        out.append((Ja, Jb, w))
    return out


def dense_J(F, n, x, ia, ib, meas, sq, huber_a, anchor, zero):
    cols = [v for v in range(n) if v != anchor]
    pos = {v: k for k, v in enumerate(cols)}
    rows = edge_jacobians(F, x, ia, ib, meas, sq, huber_a)
    J = [[zero] * (3 * len(cols)) for _ in range(3 * len(ia))]
    for e, (Ja, Jb, _) in enumerate(rows):
        for v, blk in ((ia[e], Ja), (ib[e], Jb)):
            if v == anchor:
                continue
            for i in range(3):
                for j in range(3):
                    J[3 * e + i][3 * pos[v] + j] = blk[i][j]
    return J, cols, [float(w) for _, _, w in rows]


def block_rel_err(got, want):
    """worst block of max|got - want| / max|want| over blocks with a non-zero truth"""
    worst = 0.0
    for g, w in zip(got, want):
        m = np.abs(w).max()
        if m > 0:
            worst = max(worst, float(np.abs(g - w).max() / m))
    return worst


def float64_blocks(n, x, ia, ib, meas, sq, huber_a, anchor):
    J, cols, _ = dense_J(float, n, x, ia, ib, meas, sq, huber_a, anchor, 0.0)
    J = np.array(J)
    H = J.T @ J
    Hi = np.linalg.inv(H)
    blocks = np.zeros((n, 3, 3))
    for k, v in enumerate(cols):
        blocks[v] = Hi[3 * k:3 * k + 3, 3 * k:3 * k + 3]
    return blocks, float(np.linalg.cond(H))


def run_case(case):
    import mpmath as mp

    name, n, loops, weight, anchor, huber_a, seed = case
    mp.mp.dps = 60
    _, x0, ia, ib, meas, sq = make_graph(n, loops, seed=seed, loop_weight=weight)
    meas = meas.copy()
    if huber_a > 0:
        meas[-1] += [3.0, -2.0, 0.4]   # a false loop closure that Huber down-weights
    J, cols, w = dense_J(mp.mpf, n, x0, ia, ib, meas, sq, huber_a, anchor, mp.mpf(0))
    J = mp.matrix(J)
    Hi = mp.inverse(J.T * J)
    blocks = np.zeros((n, 3, 3))
    for k, v in enumerate(cols):
        for i in range(3):
            for j in range(3):
                blocks[v, i, j] = float(Hi[3 * k + i, 3 * k + j])
    b64, cond = float64_blocks(n, x0, ia, ib, meas, sq, huber_a, anchor)
    err = block_rel_err(b64, blocks)
    print("%-16s n %d loops %d weight %g anchor %d huber %g: cond(H) %.2e err_numpy %.2e min loss weight %.3f" % (
        name, n, len(loops), weight, anchor, huber_a, cond, err, min(w)), flush=True)
    return name, dict(x=x0, id_begin=ia, id_end=ib, meas=meas, sqrt_info=sq, anchor=np.int32(anchor), huber_a=np.float64(huber_a),
                      cov=blocks, err_numpy=np.float64(err), cond=np.float64(cond))


def main():
    out = {}
    with ProcessPoolExecutor(max_workers=min(len(CASES), os.cpu_count() or 1)) as ex:
        for name, arrays in ex.map(run_case, CASES):
            for k, v in arrays.items():
                out["%s__%s" % (name, k)] = v
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "posegraph_cov_01.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
