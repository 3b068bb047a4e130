"""Dense float64 references for the pose-graph marginal covariances (test infrastructure, numpy only): the edge
Jacobians of PoseGraph2dErrorTerm written out, J over the used edges with the anchor's columns deleted, and two ways to
(J^T J)^-1 -- the normal equations and a QR factor of J (which sees cond(J) rather than its square)."""
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
    """The recipe of tests/test_posegraph.py::make_graph: circular drive, noisy odometry edges, dead-reckoned poses."""
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


def used_edges(ia, ib, max_update_index):
    ia, ib = np.asarray(ia), np.asarray(ib)
    return np.nonzero((ia + 1 == ib) | (ib <= max_update_index))[0]   # global_fuser.cpp:32


def dense_jacobian(x, ia, ib, meas, sq, max_update_index, anchor, huber_a=0.0):
    """(J, var): J [3 E_used][3 len(var)], var = poses a used edge touches, minus the anchor, ascending."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    sq = np.asarray(sq, dtype=np.float64).reshape(-1, 3, 3)
    meas = np.asarray(meas, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    anchor = n - 1 if anchor == -1 else anchor
    use = used_edges(ia, ib, max_update_index)
    touched = np.zeros(n, bool)
    touched[np.asarray(ia)[use]] = True
    touched[np.asarray(ib)[use]] = True
    touched[anchor] = False
    var = np.nonzero(touched)[0]
    pos = {int(v): k for k, v in enumerate(var)}
    J = np.zeros((3 * len(use), 3 * len(var)))
    for r, e in enumerate(use):
        a, b = int(ia[e]), int(ib[e])
        pa, pb = x[a], x[b]
        s, c = np.sin(pa[2]), np.cos(pa[2])
        dx, dy = pb[0] - pa[0], pb[1] - pa[1]
        A = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
        B = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        w = 1.0
        if huber_a > 0:   # sqrt(rho') of ceres::HuberLoss(a); ceres::Covariance applies the loss by default
            ang = (pb[2] - pa[2]) - meas[e][2]
            ev = np.array([(c * dx + s * dy) - meas[e][0], (-s * dx + c * dy) - meas[e][1], ang - 2 * np.pi * np.floor((ang + np.pi) / (2 * np.pi))])
            sn = float(np.sum((sq[e] @ ev) ** 2))
            if sn > huber_a * huber_a:
                w = np.sqrt(huber_a / np.sqrt(sn))
        if a in pos:
            J[3 * r:3 * r + 3, 3 * pos[a]:3 * pos[a] + 3] = w * (sq[e] @ A)
        if b in pos:
            J[3 * r:3 * r + 3, 3 * pos[b]:3 * pos[b] + 3] = w * (sq[e] @ B)
    return J, var


def blocks_of(n, var, sigma):
    out = np.zeros((n, 3, 3))
    for k, v in enumerate(var):
        out[v] = sigma[3 * k:3 * k + 3, 3 * k:3 * k + 3]
    return out


def cov_normal(n, J, var):
    """plain float64 np.linalg.inv(J^T J)"""
    return blocks_of(n, var, np.linalg.inv(J.T @ J))


def cov_qr(n, J, var):
    """R = qr(J), Sigma = R^-1 R^-T"""
    from scipy.linalg import solve_triangular

    R = np.linalg.qr(J, mode="r")
    Ri = solve_triangular(R, np.eye(R.shape[0]), lower=False)
    return blocks_of(n, var, Ri @ Ri.T)


def block_rel_err(got, want):
    """worst block of max|got - want| / max|want| over the blocks with a non-zero truth"""
    worst = 0.0
    for g, w in zip(got, want):
        m = np.abs(w).max()
        if m > 0:
            worst = max(worst, float(np.abs(g - w).max() / m))
    return worst


def dense_covariance(x, ia, ib, meas, sq, max_update_index, anchor=-1, huber_a=0.0):
    """[N][3][3] through the QR route; ValueError("rank deficient") when J has no full column rank."""
    n = len(x)
    J, var = dense_jacobian(x, ia, ib, meas, sq, max_update_index, anchor, huber_a)
    if J.shape[1] == 0:
        return np.zeros((n, 3, 3))
    if J.shape[0] < J.shape[1] or np.linalg.matrix_rank(J) < J.shape[1]:
        raise ValueError("rank deficient")
    return cov_qr(n, J, var)
