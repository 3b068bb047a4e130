"""randt_search_global_batch(_dev): the correlative search of randt_search_global for many pairs in one call, the level loop on
the device.  The yardstick is the single call on the same context -- poses, evaluation counts and minima bit for bit -- and, for
a batch of one, the CPU oracle at the bars of test_gpu_search_params.py.  The unmarked tests pin, on the oracle alone, that the
seven pairs do what the GPU tests need them to do (descend, dedupe, stay at the sentinel, overflow a small node table), and the
ABI (struct layout, refused arguments)."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import _capi, host, synth
from test_gpu_search_params import FAR_START, IDENTITY, SENTINEL, level1_grid, search_case
from util import GpuRig, oracle_scan_map, oracle_submap, problem, to_oracle_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, N = 5, 7                                                        # scans 5..11: both submaps, moving_first != 0
OFFSETS = ((0.9, -0.7, 0.1), (0.9, -0.7, 0.1), (-0.6, 0.5, -0.08), (0.3, 0.2, 0.05), None, (-1.1, 0.4, 0.12), (0.5, -0.9, -0.1))
WL = np.array([4.5, 3.0, 4.5, 0.3, 4.5, 2.0, 4.5])
WA = np.array([0.45, 0.3, 0.45, 0.06, 0.45, 0.45, 0.2])
LEVEL1 = [180, 48, 180, 1, 180, 45, 72]
N_EVALS = {(-1.0, 2): LEVEL1, (2.0, 2): [300, 170, 397, 27, 180, 189, 147], (1e30, 2): [4572, 1232, 4572, 27, 180, 1143, 1872],
           (2.0, 1): [720, 192, 720, 1, 720, 180, 288]}
THRESHOLDS = (-1.0, 2.0, 1e30)


def starts():
    truth = problem()["truth"]
    return np.array([FAR_START if off is None else synth.pose3_to_pose4(truth[FIRST + p] + np.array(off)) for p, off in enumerate(OFFSETS)])


def fixed_of():
    return np.ascontiguousarray(problem()["submap_of"][FIRST:FIRST + N], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def oracle_maps():
    prob = problem()
    return [oracle_submap(sm) for sm in prob["submaps"]], [oracle_scan_map(prob["scans"][FIRST + p]) for p in range(N)]


@functools.lru_cache(maxsize=None)
def oracle_answers(thr, n_iter):
    subs, scans = oracle_maps()
    bp = po.bnb_params(cost_threshold=thr, n_iter=n_iter)
    st, fo = starts(), fixed_of()
    return [po.search_global_bnb(subs[fo[p]], scans[p], po.default_params(), bp, st[p], 1.5, float(WL[p]), float(WA[p])) for p in range(N)]


# ---- CPU: the conditions ------------------------------------------------------------------------------------------------
def test_oracle_conditions(built):
    assert set(fixed_of()) == {0, 1}
    for (thr, n_iter), want in N_EVALS.items():
        got = oracle_answers(thr, n_iter)
        assert [ne for _, _, ne in got] == want, (thr, n_iter, [ne for _, _, ne in got])
    assert [len(level1_grid(starts()[p], po.bnb_params(), WL[p], WA[p])) for p in range(N)] == LEVEL1
    for mc, t4, _ in oracle_answers(-1.0, 2):
        assert mc == SENTINEL and np.array_equal(t4, IDENTITY)
    at2 = oracle_answers(2.0, 2)
    assert sum(ne > l1 for (_, _, ne), l1 in zip(at2, LEVEL1)) >= 5
    assert sum(mc == SENTINEL for mc, _, _ in at2) >= 1 and at2[4][0] == SENTINEL          # pair 4: NaN costs
    assert sum(mc < SENTINEL for mc, _, _ in at2) >= 5
    big = [ne for _, _, ne in oracle_answers(1e30, 2)]
    assert any(ne < l1 + 27 * l1 for ne, l1 in zip(big, LEVEL1) if ne > l1)                # the dedupe removed children
    assert max(big) <= 8192 and [p for p in range(N) if big[p] > 2048] == [0, 2]


# ---- CPU: the ABI -------------------------------------------------------------------------------------------------------
def test_bnb_result_layout_matches_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "randt.h"\n'
                    'int main(){printf("%zu %zu %zu %zu\\n", sizeof(randt_bnb_result), offsetof(randt_bnb_result, min_cost),'
                    " offsetof(randt_bnb_result, n_evals), offsetof(randt_bnb_result, status)); return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [16, 0, 8, 12]
    assert C.sizeof(_capi.BnbResult) == 16 == _capi.BNB_RESULT_DTYPE.itemsize
    assert (_capi.BnbResult.min_cost.offset, _capi.BnbResult.n_evals.offset, _capi.BnbResult.status.offset) == (0, 8, 12)
    assert [_capi.BNB_RESULT_DTYPE.fields[f][1] for f in ("min_cost", "n_evals", "status")] == [0, 8, 12]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(built):
    r = GpuRig(problem(), scan_cap=512)
    r.build_submaps()
    r.build_scans()
    return r


def run_batch(rig, mp, bp, order=None, max_nodes=8192):
    """The _dev entry on device tensors; order: which of the seven pairs, in which order (the scans are copied into a contiguous
    batch in that order).  Returns (poses, BNB_RESULT_DTYPE records)."""
    torch = rig.torch
    order = list(range(N)) if order is None else list(order)
    n = len(order)
    if order == list(range(N)):
        moving, first = rig.scan_maps, FIRST
    else:
        moving, first = R.Maps(rig.ctx, n + 1, rig.mapp, rig.scan_cap, with_grid=False), 1
        for i, p in enumerate(order):
            moving.copy_from(rig.scan_maps, dst_first=1 + i, src_first=FIRST + p, count=1)
    t = torch.from_numpy(np.ascontiguousarray(starts()[order])).to(rig.dev)
    fidx = torch.from_numpy(np.ascontiguousarray(fixed_of()[order])).to(rig.dev)
    res = torch.full((n, 16), 0x5a, dtype=torch.uint8, device=rig.dev)
    host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, moving, first, n, mp, bp, t, res, 1.5, WL[order], WA[order], max_nodes)
    rig.ctx.synchronize()
    return t.cpu().numpy(), res.cpu().numpy().view(_capi.BNB_RESULT_DTYPE).reshape(n)


_SINGLE = {}


def run_single(rig, mp_over, bp_over):
    """host.search_global per pair on the same context, computed once per parameter set."""
    key = (tuple(sorted(mp_over.items())), tuple(sorted(bp_over.items())))
    if key not in _SINGLE:
        mp, bp = R.default_matcher_params(**mp_over), host.bnb_params(**bp_over)
        st, fo = starts(), fixed_of()
        _SINGLE[key] = [host.search_global(rig.ctx, rig.submaps, int(fo[p]), rig.scan_maps, FIRST + p, mp, bp, st[p], 1.5, float(WL[p]), float(WA[p]))
                        for p in range(N)]
    return _SINGLE[key]


def assert_same(single, poses, res, pairs=None):
    for i, p in enumerate(range(N) if pairs is None else pairs):
        mc, t4, ne = single[p]
        assert res["status"][i] == 0, (p, res[i])
        assert res["n_evals"][i] == ne, (p, res["n_evals"][i], ne)
        assert np.array_equal(poses[i].view(np.uint64), t4.view(np.uint64)), (p, poses[i], t4)
        assert np.float64(res["min_cost"][i]).view(np.uint64) == np.float64(mc).view(np.uint64), (p, res["min_cost"][i], mc)


def host_nodes(start, bp, swl, swa):
    """Every node of a search that admits everything, in FIFO order, from the oracle's pose product: the level-1 grid, then per
    level the children whose key was never generated before."""
    astep = math.acos(1 - ((bp.csm_linear_step * bp.csm_linear_step) / (2 * bp.csm_max_px_accurate_range * bp.csm_max_px_accurate_range)))
    key = lambda x: tuple(float(np.float32(v) + np.float32(0.0)) for v in x)                # -0.0f == 0.0f
    level = [np.array(x) for x in level1_grid(start, bp, swl, swa)]
    nodes, seen = list(level), {key(x) for x in level}
    for lv in range(1, bp.csm_n_iter):
        cls, nxt = 2.0 ** lv * bp.csm_linear_step, []
        deltas = []
        for tx in (-cls, -cls + cls, -cls + cls + cls):
            for ty in (-cls, -cls + cls, -cls + cls + cls):
                for a in (-astep, -astep + astep, -astep + astep + astep):
                    c, s = math.cos(a), math.sin(a)                  # libm, like the C loops
                    n = math.sqrt(c * c + s * s)
                    deltas.append([c / n, s / n, tx, ty])
        for x in level:
            for d in deltas:
                y = np.array(po.se2_mul(x, d))
                if key(y) not in seen:
                    seen.add(key(y))
                    nxt.append(y)
        nodes += nxt
        level = nxt
    return np.array(nodes)


@pytest.mark.gpu
def test_device_pose_product_is_the_hosts(rig):
    """T0: all 4572 node poses of pair 0 at a threshold that admits everything, against the oracle's se2_mul (whose bits the
    single call's replay has: test_search_matches_oracle), downloaded through the debug hook."""
    lib = _capi.load()
    bp = host.bnb_params(cost_threshold=1e30)
    want = host_nodes(starts()[0], bp, WL[0], WA[0])
    assert len(want) == N_EVALS[(1e30, 2)][0] == 4572
    run_batch(rig, R.default_matcher_params(), bp)
    got, n = np.zeros((8192, 4)), C.c_int(0)
    lib.randt_debug_search_batch_nodes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert lib.randt_debug_search_batch_nodes(rig.ctx._h, 0, got.ctypes.data, 8192, C.byref(n)) == 0
    assert n.value == len(want)
    differ = np.nonzero((got[:n.value].view(np.uint64) != want.view(np.uint64)).any(1))[0]
    print("pose product: %d of %d nodes differ from the host's" % (len(differ), n.value))
    assert len(differ) == 0, (differ[:5], got[differ[:1]], want[differ[:1]])


CASES = [(dict(), dict(cost_threshold=t)) for t in THRESHOLDS] + [
    (dict(), dict(cost_threshold=2.0, n_iter=1)), (dict(), dict(cost_threshold=2.0, n_iter=3, linear_step=0.25)),
    (dict(use_intensity=0), dict(cost_threshold=2.0)), (dict(use_intensity=1), dict(cost_threshold=2.0)),
    (dict(lookup_mahalanobis=0), dict(cost_threshold=2.0)), (dict(loss_alpha=1.0), dict(cost_threshold=2.0)),
    (dict(loss_alpha=-2.0), dict(cost_threshold=1e30))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s=%g" % kv for kv in list(c[0].items()) + list(c[1].items())))
def test_batch_equals_the_single_call(rig, case):
    """T1: d_trans4 rows, n_evals and min_cost bit-equal to host.search_global per pair, every status 0, max_nodes 8192."""
    mp_over, bp_over = case
    single = run_single(rig, mp_over, bp_over)
    if mp_over == {} and (bp_over["cost_threshold"], bp_over.get("n_iter", 2)) in N_EVALS and "linear_step" not in bp_over:
        assert [ne for _, _, ne in single] == N_EVALS[(bp_over["cost_threshold"], bp_over.get("n_iter", 2))]
    poses, res = run_batch(rig, R.default_matcher_params(**mp_over), host.bnb_params(**bp_over))
    print("n_evals", res["n_evals"].tolist(), "min", res["min_cost"].tolist())
    assert_same(single, poses, res)


@pytest.mark.gpu
def test_batch_of_one_equals_the_oracle(rig):
    """T1, the rest: search_case(0, 0) -- pair (submap 0, scan 0) at a threshold in a gap of its level-1 costs -- as a batch of
    one, at the oracle bars of test_search_matches_oracle."""
    torch = rig.torch
    c = search_case(0, 0)
    omc, ot4, one = c["oracle"]
    t = torch.from_numpy(np.ascontiguousarray(c["start"][None])).to(rig.dev)
    fidx = torch.zeros(1, dtype=torch.int32, device=rig.dev)
    res = torch.zeros((1, 16), dtype=torch.uint8, device=rig.dev)
    host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, rig.scan_maps, 0, 1, c["mp"], host.bnb_params(cost_threshold=c["thr"]), t, res, 1.5,
                                 c["swl"], c["swa"])
    rig.ctx.synchronize()
    r = res.cpu().numpy().view(_capi.BNB_RESULT_DTYPE)[0]
    assert r["status"] == 0 and r["n_evals"] == one > c["n_level1"]
    assert np.array_equal(t.cpu().numpy()[0], ot4)
    assert np.isclose(r["min_cost"], omc, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_overflow_is_flagged_and_contained(rig):
    """T2: max_nodes 2048 at a threshold that admits everything: pairs 0 and 2 (4572 nodes) stop with status 1 and keep their
    guess, the others are untouched by it; the synchronous convenience searches those two again and returns everything."""
    single = run_single(rig, {}, dict(cost_threshold=1e30))
    mp, bp = R.default_matcher_params(), host.bnb_params(cost_threshold=1e30)
    poses, res = run_batch(rig, mp, bp, max_nodes=2048)
    assert res["status"].tolist() == [1, 0, 1, 0, 0, 0, 0]
    st = starts()
    for p in (0, 2):
        assert np.array_equal(poses[p].view(np.uint64), st[p].view(np.uint64))
        assert 180 <= res["n_evals"][p] <= 2048
    rest = [1, 3, 4, 5, 6]
    assert_same(single, poses[rest], res[rest], rest)
    mc, t4, ne = host.search_global_batch(rig.ctx, rig.submaps, fixed_of(), rig.scan_maps, FIRST, mp, bp, st, 1.5, WL, WA, max_nodes=2048)
    for p in range(N):
        assert ne[p] == single[p][2] and np.array_equal(t4[p].view(np.uint64), single[p][1].view(np.uint64))
        assert np.float64(mc[p]).view(np.uint64) == np.float64(single[p][0]).view(np.uint64)
    # the default bound holds all seven: no second search, the same answers
    mc, t4, ne = host.search_global_batch(rig.ctx, rig.submaps, fixed_of(), rig.scan_maps, FIRST, mp, bp, st, 1.5, WL, WA)
    assert ne.tolist() == [s[2] for s in single] and np.array_equal(t4, np.array([s[1] for s in single]))


@pytest.mark.gpu
def test_overflow_and_empty_grids_at_level_one(rig):
    """T2, level 1: no pair of the batch has a grid the seed launch could be sized from.  max_nodes 40 is below six of the seven
    level-1 counts (pair 3 has one node and 27 evaluations: it fits); max_nodes 20 and a batch of one flag everything; a
    non-positive angular or a negative linear window gives an empty grid: the single call's identity and sentinel, 0
    evaluations."""
    torch = rig.torch
    mp, bp = R.default_matcher_params(), host.bnb_params(cost_threshold=2.0)
    single = run_single(rig, {}, dict(cost_threshold=2.0))
    st, fo = starts(), fixed_of()
    poses, res = run_batch(rig, mp, bp, max_nodes=40)
    assert res["status"].tolist() == [1, 1, 1, 0, 1, 1, 1] and res["n_evals"].tolist() == [0, 0, 0, 27, 0, 0, 0]
    assert_same(single, poses[[3]], res[[3]], [3])
    for max_nodes, order in ((20, list(range(N))), (40, [0])):      # every pair flagged (pair 3: at its expansion), a batch of one
        whole = order == list(range(N))
        poses, res = run_batch(rig, mp, bp, order=None if whole else order, max_nodes=max_nodes)
        assert (res["status"] == 1).all(), (max_nodes, res)
        assert res["n_evals"].tolist() == [1 if p == 3 else 0 for p in order]
        for i, p in enumerate(order):
            assert np.array_equal(poses[i].view(np.uint64), st[p].view(np.uint64))          # the guess is kept
            assert p == 3 or res["min_cost"][i] == SENTINEL
        moving, first = (rig.scan_maps, FIRST) if whole else (_contiguous(rig, order), 0)
        mc, t4, ne = host.search_global_batch(rig.ctx, rig.submaps, fo[order], moving, first, mp, bp, st[order], 1.5, WL[order], WA[order],
                                              max_nodes=max_nodes)
        for i, p in enumerate(order):
            assert ne[i] == single[p][2] and np.array_equal(t4[i].view(np.uint64), single[p][1].view(np.uint64))
            assert np.float64(mc[i]).view(np.uint64) == np.float64(single[p][0]).view(np.uint64)
    # empty grids: every pair, and one pair among pairs that search
    for wl, wa in ((WL, np.zeros(N)), (WL, -WA), (-WL, WA)):
        t = torch.from_numpy(np.ascontiguousarray(st)).to(rig.dev)
        fidx = torch.from_numpy(fo).to(rig.dev)
        r = torch.full((N, 16), 0x5a, dtype=torch.uint8, device=rig.dev)
        host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, N, mp, bp, t, r, 1.5, wl, wa)
        rig.ctx.synchronize()
        r = r.cpu().numpy().view(_capi.BNB_RESULT_DTYPE).reshape(N)
        assert (r["status"] == 0).all() and (r["n_evals"] == 0).all() and (r["min_cost"] == SENTINEL).all()
        assert np.array_equal(t.cpu().numpy(), np.tile(IDENTITY, (N, 1)))
        mc1, t1, ne1 = host.search_global(rig.ctx, rig.submaps, int(fo[0]), rig.scan_maps, FIRST, mp, bp, st[0], 1.5, float(wl[0]), float(wa[0]))
        assert mc1 == SENTINEL and ne1 == 0 and np.array_equal(t1, IDENTITY)
    wa = WA.copy()
    wa[2] = 0.0
    t = torch.from_numpy(np.ascontiguousarray(st)).to(rig.dev)
    r = torch.zeros((N, 16), dtype=torch.uint8, device=rig.dev)
    host.search_global_batch_dev(rig.ctx, rig.submaps, torch.from_numpy(fo).to(rig.dev), rig.scan_maps, FIRST, N, mp, bp, t, r, 1.5, WL, wa)
    rig.ctx.synchronize()
    r, poses = r.cpu().numpy().view(_capi.BNB_RESULT_DTYPE).reshape(N), t.cpu().numpy()
    assert r["n_evals"][2] == 0 and r["min_cost"][2] == SENTINEL and np.array_equal(poses[2], IDENTITY) and r["status"][2] == 0
    rest = [0, 1, 3, 4, 5, 6]
    assert_same(single, poses[rest], r[rest], rest)


def _contiguous(rig, order):
    m = R.Maps(rig.ctx, len(order), rig.mapp, rig.scan_cap, with_grid=False)
    for i, p in enumerate(order):
        m.copy_from(rig.scan_maps, dst_first=i, src_first=FIRST + p, count=1)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("order", [tuple(reversed(range(N))), tuple(range(N)) + (0,)], ids=["reversed", "pair0_twice"])
def test_pairs_do_not_depend_on_their_neighbours(rig, order):
    """T3: the same pairs in another order / with a duplicate: every pair's result is unchanged."""
    for thr in (2.0, 1e30):
        single = run_single(rig, {}, dict(cost_threshold=thr))
        poses, res = run_batch(rig, R.default_matcher_params(), host.bnb_params(cost_threshold=thr), order=order)
        assert_same(single, poses, res, order)


@pytest.mark.gpu
def test_no_host_in_the_loop(rig):
    """T4: a warmed-up _dev call allocates nothing and waits for nothing, and its poses feed register_batch on the same stream
    without a synchronisation in between: the result of search_global -> register_pair per pair, bit for bit."""
    torch = rig.torch
    mp, bp = R.default_matcher_params(), host.bnb_params(cost_threshold=2.0)
    st, fo = starts(), fixed_of()
    want = []
    for p in range(N):
        _, g, _ = host.search_global(rig.ctx, rig.submaps, int(fo[p]), rig.scan_maps, FIRST + p, mp, bp, st[p], 1.5, float(WL[p]), float(WA[p]))
        want.append(host.register_pair(rig.ctx, rig.submaps, int(fo[p]), rig.scan_maps, FIRST + p, mp, g))
    fidx = torch.from_numpy(fo).to(rig.dev)
    h_t = torch.from_numpy(np.ascontiguousarray(st))
    t = h_t.to(rig.dev)
    bres = torch.zeros((N, 16), dtype=torch.uint8, device=rig.dev)
    rres = torch.zeros((N, 64), dtype=torch.uint8, device=rig.dev)
    host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, N, mp, bp, t, bres, 1.5, WL, WA)      # warm-up: the workspace grows
    host.register_batch(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, N, mp, t, rres)
    rig.ctx.synchronize()
    t.copy_(h_t)
    rig.ctx.synchronize()
    before = rig.ctx.pool_stats()
    host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, N, mp, bp, t, bres, 1.5, WL, WA)
    after = rig.ctx.pool_stats()
    host.register_batch(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, N, mp, t, rres)
    rig.ctx.synchronize()
    assert after["device_allocs"] == before["device_allocs"] and after["stream_syncs"] == before["stream_syncs"], (before, after)
    assert (bres.cpu().numpy().view(_capi.BNB_RESULT_DTYPE)["status"] == 0).all()
    poses, recs = t.cpu().numpy(), rres.cpu().numpy().view(_capi.RESULT_DTYPE).reshape(N)
    for p in range(N):
        assert np.array_equal(poses[p].view(np.uint64), want[p][0].view(np.uint64)), (p, poses[p], want[p][0])
        assert recs[p].tobytes() == want[p][1].tobytes(), (p, recs[p], want[p][1])


# ---- the argument checks proper need a context, so a device ----------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_arguments_are_refused(rig):
    """T5: n_pairs = 0, max_nodes = 0, a NaN window, csm_linear_step <= 0 -- refused before anything is enqueued."""
    torch = rig.torch
    mp = R.default_matcher_params()
    t = torch.from_numpy(np.ascontiguousarray(starts())).to(rig.dev)
    fidx = torch.from_numpy(fixed_of()).to(rig.dev)
    res = torch.zeros((N, 16), dtype=torch.uint8, device=rig.dev)

    def call(n=N, bp=host.bnb_params(), wl=WL, wa=WA, max_nodes=8192):
        host.search_global_batch_dev(rig.ctx, rig.submaps, fidx, rig.scan_maps, FIRST, n, mp, bp, t, res, 1.5, wl[:max(n, 1)], wa[:max(n, 1)], max_nodes)

    bad_wl = WL.copy()
    bad_wl[3] = np.nan
    for kw in (dict(n=0), dict(max_nodes=0), dict(wl=bad_wl), dict(wa=bad_wl), dict(bp=host.bnb_params(linear_step=0.0)),
               dict(bp=host.bnb_params(linear_step=-0.4)), dict(bp=host.bnb_params(n_iter=17))):
        with pytest.raises(R.RandtError) as e:
            call(**kw)
        assert e.value.status == _capi.ERR_INVALID, kw
    with pytest.raises(R.RandtError):
        host.search_global_batch(rig.ctx, rig.submaps, fixed_of(), rig.scan_maps, FIRST, mp, host.bnb_params(linear_step=0.0), starts(), 1.5, WL, WA)
    bad_idx = fixed_of().copy()
    bad_idx[5] = rig.n_sub                                                                 # a fixed map that does not exist
    for idx in (bad_idx, -1 - fixed_of()):
        with pytest.raises(R.RandtError) as e:
            host.search_global_batch(rig.ctx, rig.submaps, idx, rig.scan_maps, FIRST, mp, host.bnb_params(), starts(), 1.5, WL, WA)
        assert e.value.status == _capi.ERR_INVALID
    lib, bp, w = _capi.load(), host.bnb_params(), np.array([4.5])                          # no context at all
    assert lib.randt_search_global_batch_dev(None, rig.submaps._h, _capi.C.c_void_p(fidx.data_ptr()), rig.scan_maps._h, FIRST, 1, C.byref(mp), C.byref(bp),
                                             1.5, w.ctypes.data, w.ctypes.data, 8192, _capi.C.c_void_p(t.data_ptr()),
                                             _capi.C.c_void_p(res.data_ptr())) == _capi.ERR_INVALID
    rig.ctx.synchronize()
    assert np.array_equal(t.cpu().numpy(), starts())                                       # nothing ran
    call()                                                                                 # the same call with valid arguments runs
    rig.ctx.synchronize()
    assert not np.array_equal(t.cpu().numpy(), starts())
