"""SURVEY row f-3 beyond the shipped defaults: k_eval_cost<2> and <3>, every loss branch, non-unit poses, map indices other
than 0, and randt_search_global over the parameters the facade's estimateTransformGlobalBNB exposes (intensity dimension,
loss shape, lookup metric, scale, windows, steps, levels).  References: the CPU oracle, and for the cost a float64 numpy
definition that shares nothing with it.  The unmarked tests pin the oracle and the conditions under which a search parity run
proves something, so they run without a GPU."""
import functools
import math

import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import host, synth
from util import GpuRig, oracle_scan_map, oracle_submap, problem, to_oracle_params

KS, DS, ALPHAS = (1, 4, 6), (2, 3), (-2.0, -1.5, -1.0, 0.0, 0.05, 1.0, 2.0)
SENTINEL = 100000.0
IDENTITY = [1.0, 0.0, 0.0, 0.0]
FAR_START = np.array([np.cos(0.3), np.sin(0.3), 400.0, -300.0])          # no moving cell finds a fixed cell from here


@functools.lru_cache(maxsize=None)
def scene(sub_i=0, scan_i=0):
    prob = problem()
    return oracle_submap(prob["submaps"][sub_i]), oracle_scan_map(prob["scans"][scan_i])


def cloud(scan_i, n, seed=0):
    """n poses scattered around a scan's true pose."""
    rng = np.random.default_rng(seed)
    return synth.pose3_to_pose4(problem()["truth"][scan_i] + rng.normal(0, [0.5, 0.5, 0.1], (n, 3)))


# ---- the cost from its definition: 1/2 sum rho(d^T (R Sm R^T + Sf)^-1 d) over the first dim components (ceres_residuals.h:421-552),
# rho = BarronLoss(a, alpha) at mu = 1 as barron() of tests/golden/make_independent.py writes it
def barron_rho(z, a, alpha):
    b = a * a
    if alpha >= 2.0:
        return z
    if abs(alpha) <= 0.05:
        return b * np.log(1.0 + z / b)
    f = abs(alpha - 2.0)
    return b * f / alpha * ((z * (2.0 / (b * f)) + 1.0) ** (0.5 * alpha) - 1.0)


def full(cov):
    c = np.asarray(cov, dtype=np.float64).reshape(-1, 6)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def cost_definition(fc, mc, corr, poses4, dim, scale, alpha):
    mi, kk = np.nonzero(corr[:len(mc)] >= 0)
    fi = corr[mi, kk]
    out = np.zeros(len(poses4))
    if len(mi) == 0:
        return out, 0
    mm, fm = mc["mean"][mi].astype(np.float64)[:, :dim], fc["mean"][fi].astype(np.float64)[:, :dim]
    Sm, Sf = full(mc["cov"][mi])[:, :dim, :dim], full(fc["cov"][fi])[:, :dim, :dim]
    for p, x in enumerate(np.asarray(poses4, dtype=np.float64)):
        c, s = x[:2] / np.hypot(x[0], x[1])
        Rm = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])[:dim, :dim]
        d = mm @ Rm.T + np.array([x[2], x[3], 0.0])[:dim] - fm
        C = Rm @ Sm @ Rm.T + Sf
        z = np.einsum("ni,ni->n", d, np.linalg.solve(C, d[..., None])[..., 0])
        out[p] = 0.5 * barron_rho(z, scale, alpha).sum()
    return out, len(mi)


def test_oracle_cost_matches_numpy_definition(built):
    """B1.  Measured over this grid: 2.2e-15 relative at most (9.5e-16 over k in {1, 4} and the integer shapes); the bar is 1e-13."""
    sub, scan = scene()
    fc, mc = sub.cells(), scan.cells()
    poses = cloud(0, 20)
    g = synth.pose3_to_pose4(problem()["guess"][0])
    worst = 0.0
    for k in KS:
        for dim in DS:
            corr, n = po.associate(sub, scan, g, k, True, dim == 3)
            assert n > 40 * k
            for alpha in ALPHAS:
                ref, n_ref = cost_definition(fc, mc, corr, poses, dim, 1.5, alpha)
                got, n_got = po.eval_cost_batch(sub, scan, corr, poses, 1.5, alpha, int(dim == 3))
                assert n_got == n_ref == n and ref.min() > 0
                worst = max(worst, np.abs(got / ref - 1.0).max())
                assert np.allclose(got, ref, rtol=1e-13, atol=0), (k, dim, alpha, np.abs(got / ref - 1.0).max())
    print("oracle vs numpy definition: worst relative difference %.3g" % worst)
    # alpha = 0 and 0.05 share the log branch by design (|alpha| <= 0.05), and it is a branch of its own
    corr, _ = po.associate(sub, scan, g, 4)
    c0, c005, c1 = (po.eval_cost_batch(sub, scan, corr, poses, 1.5, a)[0] for a in (0.0, 0.05, 0.1))
    assert np.array_equal(c0, c005) and not np.allclose(c0, c1, rtol=1e-3)
    # a pose row of any length is the pose of its direction: exactly, in the oracle
    for f in (1.7, 0.3):
        scaled = poses.copy()
        scaled[:, :2] *= f
        assert np.array_equal(po.eval_cost_batch(sub, scan, corr, scaled)[0], po.eval_cost_batch(sub, scan, corr, poses)[0])


# ---- the search: where a parity run proves something -----------------------------------------------------------------
MATCHER = (dict(), dict(use_intensity=0), dict(loss_alpha=-1.0), dict(loss_alpha=0.0), dict(loss_alpha=1.0), dict(loss_alpha=2.0),
           dict(lookup_mahalanobis=0, use_intensity=0))
SEARCH = (dict(), dict(n_iter=3, linear_step=0.25), dict(n_iter=1, window_linear=2.0))
BAD = np.array([0.9, -0.7, 0.1])
# (name, matcher overrides, csm_* overrides, window arguments, start pose3 or None = truth + BAD)
EXTRA = (("range2", dict(), dict(max_px_accurate_range=2.0), (4.5, 0.45), None),
         ("fmin", dict(), dict(), (3.0, 0.3), None),                     # window arguments smaller than the csm_* windows
         ("zero_rotation", dict(), dict(), (4.5, 0.45), "zero"),
         ("near_pi", dict(), dict(), (4.5, 0.45), "pi"))


def start_pose(kind):
    t = problem()["truth"][0]
    if kind == "zero":
        return np.array([1.0, 0.0, t[0] + BAD[0], t[1] + BAD[1]])       # c = 1, s = 0 exactly
    if kind == "pi":
        return synth.pose3_to_pose4(np.array([t[0] + BAD[0], t[1] + BAD[1], np.pi - 0.01]))   # the angular window straddles pi
    return synth.pose3_to_pose4(t + BAD)


def level1_grid(start4, bp, swl, swa):
    """The three nested loops of ndt_matcher.cpp:527-541, with their running float sums."""
    swl, swa = min(swl, bp.csm_window_linear), min(swa, bp.csm_window_angular)
    step = 2.0 ** (bp.csm_n_iter - 1) * bp.csm_linear_step
    astep = math.acos(1 - ((bp.csm_linear_step * bp.csm_linear_step) / (2 * bp.csm_max_px_accurate_range * bp.csm_max_px_accurate_range)))
    poses = []
    tx = -swl / 2.0
    while tx <= swl / 2.0:
        ty = -swl / 2.0
        while ty <= swl / 2.0:
            a = -swa / 2.0
            while a < swa / 2.0:
                c, s = math.cos(a), math.sin(a)                          # libm, like the C loops; then Sophus' normalize()
                n = math.sqrt(c * c + s * s)
                poses.append(po.se2_mul(start4, [c / n, s / n, tx, ty]))
                a += astep
            ty += step
        tx += step
    return np.array(poses)


@functools.lru_cache(maxsize=None)
def search_case(m_i, s_i, extra=None):
    """One run: parameters, the threshold taken from the oracle's level-1 costs, the oracle's answers.  Everything asserted here
    is about the oracle alone."""
    sub, scan = scene()
    if extra is None:
        m_over, s_over, (swl, swa), start = MATCHER[m_i], SEARCH[s_i], (4.5, 0.45), start_pose(None)
    else:
        _, m_over, s_over, (swl, swa), kind = EXTRA[extra]
        start = start_pose(kind)
    mp = R.default_matcher_params(**m_over)
    op = to_oracle_params(mp)
    none = po.bnb_params(cost_threshold=-1.0, **s_over)                  # costs are >= 0: admits nothing
    grid = level1_grid(start, none, swl, swa)
    mc0, t0, n0 = po.search_global_bnb(sub, scan, op, none, start, 1.5, swl, swa)
    assert n0 == len(grid) and mc0 == SENTINEL and np.array_equal(t0, IDENTITY)
    corr, n_res = po.associate(sub, scan, start, 4, bool(mp.lookup_mahalanobis), bool(mp.use_intensity))
    cost, n_res2 = po.eval_cost_batch(sub, scan, corr, grid, 1.5, mp.loss_alpha, mp.use_intensity)
    assert n_res2 == n_res > 0
    s = np.sort(cost / n_res)
    i0 = int(np.ceil(0.10 * len(s)))
    cand = s[i0:i0 + 10]                                                 # the ten costs above the 10th percentile: nine gaps
    j = int(np.argmax(np.diff(cand)))
    thr = 0.5 * (cand[j] + cand[j + 1])
    gap = (cand[j + 1] - cand[j]) / thr
    assert gap >= 1e-6, gap
    bp = po.bnb_params(cost_threshold=thr, **s_over)
    omc, ot4, one = po.search_global_bnb(sub, scan, op, bp, start, 1.5, swl, swa)
    below = int((s < thr).sum())
    assert below == i0 + j + 1 and omc < SENTINEL
    if bp.csm_n_iter > 1:
        assert one > len(grid)
    else:
        assert one == len(grid)
    return dict(mp=mp, s_over=s_over, swl=swl, swa=swa, start=start, grid=grid, thr=thr, gap=gap, below=below, n_level1=len(grid),
                oracle=(omc, ot4, one))


def all_search_cases():
    return [(m, s, None) for m in range(len(MATCHER)) for s in range(len(SEARCH))] + [(0, 0, e) for e in range(len(EXTRA))]


def case_id(c):
    if c[2] is not None:
        return EXTRA[c[2]][0]
    return "-".join("%s=%g" % kv for kv in list(MATCHER[c[0]].items()) + list(SEARCH[c[1]].items())) or "defaults"


@pytest.mark.parametrize("case", all_search_cases(), ids=case_id)
def test_oracle_search_conditions(built, case):
    """B3 on the CPU: the threshold sits in a real gap of the level-1 costs, the numpy grid has the oracle's node count, and the
    oracle descends below level 1 (n_iter > 1) and finds a minimum.  At the fixed threshold 2.0 the loss shapes -1 .. 2 admit
    no node at all and a parity run would compare two sentinels."""
    c = search_case(*case)
    print("%s: threshold %.6g, gap %.2g, %d of %d level-1 nodes below, oracle n_evals %d, min cost %.6g"
          % (case_id(case), c["thr"], c["gap"], c["below"], c["n_level1"], c["oracle"][2], c["oracle"][0]))
    assert 1e-6 <= c["gap"] and c["below"] >= 0.10 * c["n_level1"]


def check_threshold_is_strict(c, level1_costs, search):
    """`current_cost < cost_threshold` (ndt_matcher.cpp:577) with the threshold ON a level-1 node's own normalised cost, as the
    implementation under test computes it: the node stays out, so the run equals the oracle's at the gap threshold just below
    (the same level-1 nodes go down; level 2 is the last one, so what else it admits there changes neither the count nor the
    minimum); one ulp higher the node is in and its children are evaluated."""
    assert c["s_over"] == {}
    cn = level1_costs(c["grid"])
    j = int(np.argsort(cn)[c["below"]])                                  # the first node above the gap
    assert cn[j] > c["thr"] and int((cn < cn[j]).sum()) == c["below"]
    omc, ot4, one = c["oracle"]
    mc, t4, ne = search(float(cn[j]))
    assert ne == one and np.array_equal(t4, ot4) and np.isclose(mc, omc, rtol=1e-12, atol=0), (ne, one, mc, omc)
    mc, t4, ne = search(float(np.nextafter(cn[j], np.inf)))
    assert ne > one, (ne, one)


def test_oracle_threshold_is_strict(built):
    sub, scan = scene()
    c = search_case(0, 0)
    op = to_oracle_params(c["mp"])
    corr, n_res = po.associate(sub, scan, c["start"], 4)
    check_threshold_is_strict(c, lambda grid: po.eval_cost_batch(sub, scan, corr, grid)[0] / n_res,
                              lambda thr: po.search_global_bnb(sub, scan, op, po.bnb_params(cost_threshold=thr), c["start"]))


def test_oracle_degenerate_search(built):
    """B4 on the CPU: a start pose where no moving cell finds a fixed cell -- 0 residuals, every normalised cost 0 / 0 = NaN,
    which is below no threshold: the sentinel, the identity and the level-1 count."""
    sub, scan = scene()
    corr, n = po.associate(sub, scan, FAR_START, 4)
    assert n == 0 and (corr < 0).all()
    cost, n_res = po.eval_cost_batch(sub, scan, corr, FAR_START[None])
    assert n_res == 0 and cost[0] == 0.0
    bp = po.bnb_params(cost_threshold=1e30)
    mc, t4, ne = po.search_global_bnb(sub, scan, po.default_params(), bp, FAR_START)
    assert mc == SENTINEL and np.array_equal(t4, IDENTITY) and ne == len(level1_grid(FAR_START, bp, 4.5, 0.45)) == 180


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(built):
    r = GpuRig(problem(), scan_cap=512)
    r.build_submaps()
    r.build_scans()
    return r


def device_corr(rig, sub_i, scan_i, guess4, mp):
    torch = rig.torch
    corr = torch.full((1, rig.scan_cap, mp.n_neighbours), -1, dtype=torch.int32, device=rig.dev)
    fidx = torch.tensor([sub_i], dtype=torch.int32, device=rig.dev)
    R.associate_batch(rig.ctx, rig.submaps, fidx, rig.scan_maps, scan_i, 1, torch.from_numpy(np.ascontiguousarray(guess4[None])).to(rig.dev), mp, corr)
    return corr


def device_cost(rig, sub_i, scan_i, corr, mp, scale, poses4, want_n=True, moving=None):
    torch = rig.torch
    cost = torch.full((len(poses4),), -7.0, dtype=torch.float64, device=rig.dev)
    nres = torch.full((1,), -7, dtype=torch.int32, device=rig.dev) if want_n else None
    host.eval_cost_batch(rig.ctx, rig.submaps, sub_i, rig.scan_maps if moving is None else moving, scan_i, corr, mp, scale,
                         torch.from_numpy(np.ascontiguousarray(poses4)).to(rig.dev), cost, nres)
    rig.ctx.synchronize()
    return cost.cpu().numpy(), (int(nres.item()) if want_n else None)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DS)
@pytest.mark.parametrize("k", KS)
def test_cost_batch_grid(rig, k, dim):
    """B2: k_eval_cost<dim> at every loss branch against the oracle AND the numpy definition, both at the existing 1e-12."""
    sub, scan = scene()
    fc, mc = sub.cells(), scan.cells()
    g = synth.pose3_to_pose4(problem()["guess"][0])
    poses = cloud(0, 20)
    for alpha in ALPHAS:
        mp = R.default_matcher_params(n_neighbours=k, use_intensity=int(dim == 3), lookup_mahalanobis=1, loss_alpha=alpha)
        corr = device_corr(rig, 0, 0, g, mp)
        ocorr, n = po.associate(sub, scan, g, k, True, dim == 3)
        hc = corr.cpu().numpy()[0]
        assert np.array_equal(hc[:len(mc)], ocorr)
        cost, nres = device_cost(rig, 0, 0, corr, mp, 1.5, poses)
        ocost, on = po.eval_cost_batch(sub, scan, ocorr, poses, 1.5, alpha, int(dim == 3))
        ncost, nn = cost_definition(fc, mc, hc, poses, dim, 1.5, alpha)
        print("k %d dim %d alpha %g: vs oracle %.3g, vs numpy %.3g" % (k, dim, alpha, np.abs(cost / ocost - 1).max(), np.abs(cost / ncost - 1).max()))
        assert nres == on == nn == n
        assert np.allclose(cost, ocost, rtol=1e-12, atol=0), (alpha, np.abs(cost / ocost - 1).max())
        assert np.allclose(cost, ncost, rtol=1e-12, atol=0), (alpha, np.abs(cost / ncost - 1).max())


@pytest.mark.gpu
@pytest.mark.parametrize("dim,alpha", [(3, -2.0), (2, -2.0), (3, 1.0), (2, 0.0)])
def test_cost_batch_edges(rig, dim, alpha):
    """B2, the rest: 1 and 300 poses, pose rows that are not unit length, no residual-count output, map indices other than 0,
    other scales, an empty table and an empty moving map."""
    prob = problem()
    scan_i = int(np.nonzero(prob["submap_of"] == 1)[0][2])                 # a scan of the SECOND submap
    assert scan_i > 0
    sub, scan = scene(1, scan_i)
    fc, mc = sub.cells(), scan.cells()
    g = synth.pose3_to_pose4(prob["guess"][scan_i])
    mp = R.default_matcher_params(use_intensity=int(dim == 3), loss_alpha=alpha)
    corr = device_corr(rig, 1, scan_i, g, mp)
    hc = corr.cpu().numpy()[0]
    ocorr, n = po.associate(sub, scan, g, 4, True, dim == 3)
    assert np.array_equal(hc[:len(mc)], ocorr) and n > 100
    for n_poses in (1, 300):
        poses = cloud(scan_i, n_poses, seed=n_poses)
        for scale in (1.5, 0.7):
            cost, nres = device_cost(rig, 1, scan_i, corr, mp, scale, poses)
            ocost, on = po.eval_cost_batch(sub, scan, ocorr, poses, scale, alpha, int(dim == 3))
            assert nres == on == n
            assert np.allclose(cost, ocost, rtol=1e-12, atol=0), (n_poses, scale, np.abs(cost / ocost - 1).max())
            assert np.allclose(cost, cost_definition(fc, mc, hc, poses, dim, scale, alpha)[0], rtol=1e-12, atol=0)
    assert alpha < 2.0 and not np.allclose(cost, device_cost(rig, 1, scan_i, corr, mp, 1.5, poses)[0], rtol=1e-3)   # the scale was used
    # the maps of index 0 are other maps: the indices were used
    assert not np.allclose(device_cost(rig, 0, 0, corr, mp, 0.7, poses)[0], cost, rtol=1e-3)
    # rows of any length: the in-kernel normalisation
    poses = cloud(scan_i, 20, seed=5)
    ocost, _ = po.eval_cost_batch(sub, scan, ocorr, poses, 1.5, alpha, int(dim == 3))
    for f in (1.7, 0.3):
        scaled = poses.copy()
        scaled[:, :2] *= f
        cost, _ = device_cost(rig, 1, scan_i, corr, mp, 1.5, scaled)
        assert np.allclose(cost, ocost, rtol=1e-12, atol=0), (f, np.abs(cost / ocost - 1).max())
    # no residual-count output
    cost, none = device_cost(rig, 1, scan_i, corr, mp, 1.5, poses, want_n=False)
    assert none is None and np.allclose(cost, ocost, rtol=1e-12, atol=0)
    # nothing associated: cost 0.0, 0 residuals
    empty = rig.torch.full_like(corr, -1)
    cost, nres = device_cost(rig, 1, scan_i, empty, mp, 1.5, poses)
    assert nres == 0 and np.array_equal(cost, np.zeros(len(poses)))
    # an empty moving map (the table is not read)
    nomap = R.Maps(rig.ctx, 3, rig.mapp, rig.scan_cap, with_grid=False)
    assert nomap.counts()[2] == 0
    cost, nres = device_cost(rig, 1, 2, corr, mp, 1.5, poses, moving=nomap)
    assert nres == 0 and np.array_equal(cost, np.zeros(len(poses)))


def run_device_search(rig, c, thr):
    bp = host.bnb_params(cost_threshold=thr, **c["s_over"])
    return host.search_global(rig.ctx, rig.submaps, 0, rig.scan_maps, 0, c["mp"], bp, c["start"], 1.5, c["swl"], c["swa"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", all_search_cases(), ids=case_id)
def test_search_matches_oracle(rig, case):
    """B3: the bars of test_hip_cost_batch_and_search_match_oracle -- n_evals equal, the pose bit for bit, the minimum at 1e-12 --
    at a threshold that admits 11-17 % of the level-1 nodes (test_oracle_search_conditions), and at one that admits none."""
    c = search_case(*case)
    omc, ot4, one = c["oracle"]
    mc, t4, ne = run_device_search(rig, c, c["thr"])
    print("%s: n_evals %d (oracle %d), min cost %.17g (oracle %.17g)" % (case_id(case), ne, one, mc, omc))
    assert ne == one, (ne, one)
    assert np.array_equal(t4, ot4), (t4, ot4)
    assert np.isclose(mc, omc, rtol=1e-12, atol=0), (mc, omc)
    mc, t4, ne = run_device_search(rig, c, -1.0)
    assert mc == SENTINEL and np.array_equal(t4, IDENTITY) and ne == c["n_level1"]


@pytest.mark.gpu
def test_search_threshold_is_strict(rig):
    c = search_case(0, 0)
    corr = device_corr(rig, 0, 0, c["start"], c["mp"])

    def level1_costs(grid):
        cost, n_res = device_cost(rig, 0, 0, corr, c["mp"], 1.5, grid)
        return cost / float(n_res)

    check_threshold_is_strict(c, level1_costs, lambda thr: run_device_search(rig, c, thr))


@pytest.mark.gpu
def test_degenerate_search(rig):
    """B4: no correspondence at the start pose (test_oracle_degenerate_search has the oracle's answer)."""
    mp = R.default_matcher_params()
    corr = device_corr(rig, 0, 0, FAR_START, mp)
    cost, nres = device_cost(rig, 0, 0, corr, mp, 1.5, FAR_START[None])
    assert nres == 0 and cost[0] == 0.0 and int((corr >= 0).sum()) == 0
    mc, t4, ne = host.search_global(rig.ctx, rig.submaps, 0, rig.scan_maps, 0, mp, host.bnb_params(cost_threshold=1e30), FAR_START)
    assert mc == SENTINEL and np.array_equal(t4, IDENTITY) and ne == 180
