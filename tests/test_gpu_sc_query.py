"""-m gpu: Scan Context place recognition for scans OUTSIDE the database (randt_sc_query_batch_dev, randt_sc_db_query,
randt_sc_db_append_node; csrc/scancontext_query.hip) and Slam.relocalize on top of it.

Two references: the existing detect entry on the database extended by the query (composition: same build, bit for bit) and
the numpy restatement tests/scancontext_ref.py through tests/sc_query_cases.py (independent: ids, yaws, distances to the
bound the detect entry is held to)."""
import numpy as np
import pytest

import randt_slam_amd as R
import sc_query_cases as sq
import scancontext_cases as cases
from randt_slam_amd import host, odometry, slam, synth
from test_scancontext_shapes import REL          # the bound the existing tests hold the detect entry to against scancontext_ref.py

pytestmark = pytest.mark.gpu

FILL_I, FILL_F = -7, -7.0


def _ctx():
    import torch

    return torch.device("cuda:0"), R.Context(0, torch.cuda.current_stream().cuda_stream)


def _gpu_query(ctx, dev, p, db, qs, prior=True, db_odom=True, n_queries=None):
    """randt_sc_query_batch_dev over all queries of `qs`; every output starts from a sentinel.  Returns numpy arrays."""
    import torch

    sp = host.sc_params(**p)
    nq = len(qs["desc"]) if n_queries is None else n_queries
    K = max(1, min(p["num_candidates"], 64))
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)                  # (a copy: the cases are read-only and shared)
    out = dict(loop=torch.full((nq,), FILL_I, dtype=torch.int32, device=dev), yaw=torch.full((nq,), FILL_F, dtype=torch.float32, device=dev),
               min_dist=torch.full((nq,), FILL_F, dtype=torch.float64, device=dev),
               cand_id=torch.full((nq, K), FILL_I, dtype=torch.int32, device=dev), cand_yaw=torch.full((nq, K), FILL_F, dtype=torch.float32, device=dev),
               cand_dist=torch.full((nq, K), FILL_F, dtype=torch.float64, device=dev))
    n_db = len(db["desc"])
    d_desc = up(db["desc"]) if n_db else torch.zeros((0, p["num_sector"], p["num_ring"]), dtype=torch.float64, device=dev)
    d_rk = up(db["rk"]) if n_db else None
    try:
        host.sc_query_batch(ctx, sp, d_desc, d_rk, up(db["pos"]) if db_odom and n_db else None, up(db["dist"]) if db_odom and n_db else None,
                            up(qs["desc"]), up(qs["rk"]), up(qs["pos"]) if prior else None, up(qs["dist"]) if prior else None,
                            out["loop"], out["yaw"], out["min_dist"], out["cand_id"], out["cand_yaw"], out["cand_dist"])
    finally:
        ctx.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
    return got


def _gpu_detect_one(ctx, dev, p, db, qs, j):
    """the composition: the database extended by query j as node n_db, num_exclude_recent = 1, detect for that node"""
    import torch

    sp = host.sc_params(**dict(p, num_exclude_recent=1))
    ext = {k: torch.from_numpy(np.concatenate([db[k], qs[k][j:j + 1]])).to(dev) for k in ("desc", "rk", "pos", "dist")}
    loop = torch.full((1,), FILL_I, dtype=torch.int32, device=dev)
    yaw = torch.full((1,), FILL_F, dtype=torch.float32, device=dev)
    md = torch.full((1,), FILL_F, dtype=torch.float64, device=dev)
    host.sc_detect_batch(ctx, sp, ext["desc"], ext["rk"], ext["pos"], ext["dist"], torch.tensor([len(db["desc"])], dtype=torch.int32, device=dev), loop, yaw, md)
    ctx.synchronize()
    return int(loop.cpu()[0]), yaw.cpu().numpy()[0], md.cpu().numpy()[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _composition(ctx, dev, p, db, qs, what):
    n_hit = 0
    for thresh in (p["dist_thresh"], -1.0):                               # -1: every match is rejected (an exact copy's distance is 0 give or take an ulp)
        pt = dict(p, dist_thresh=thresh)
        got = _gpu_query(ctx, dev, pt, db, qs)
        for j in range(len(qs["desc"])):
            lid, yaw, md = _gpu_detect_one(ctx, dev, pt, db, qs, j)
            print(what, "thresh", thresh, "query", j, "query entry", got["loop"][j], got["yaw"][j], got["min_dist"][j], "detect entry", lid, yaw, md)
            assert got["loop"][j] == lid, (what, thresh, j)
            assert _bits(got["yaw"][j:j + 1])[0] == _bits(np.array([yaw]))[0], (what, thresh, j)
            assert _bits(got["min_dist"][j:j + 1])[0] == _bits(np.array([md]))[0], (what, thresh, j, got["min_dist"][j], md)
            n_hit += lid >= 0
            if thresh < 0:
                assert lid == -1
    assert n_hit >= 1, what                                               # the accepting threshold accepted something


@pytest.mark.parametrize("name", sq.PARITY_SETS)
def test_query_equals_detect_on_the_extended_database(built, name):
    """Query q against n_db nodes == randt_sc_detect_batch_dev for node n_db of the database extended by q (exclusion 1, the
    query's position and distance): loop id, yaw bits, minimal-distance bits; with and without dist_thresh rejecting the match;
    a staged descriptor (60 x 128, and the shipped 20 x 45 over two chunks) and an unstaged one (61 x 128), the planted
    periodic descriptor (exact shift ties) among the queries."""
    import torch

    dev, ctx = _ctx()
    p, db, qs = sq.parity_case(name, False)
    lds = torch.cuda.get_device_properties(0).shared_memory_per_block
    assert cases.branches(cases.CONFIGS[name], lds)["staged"] == (name != "unstaged_min") and len(db["desc"]) >= 2
    _composition(ctx, dev, p, db, qs, name)


def test_query_equals_detect_across_chunks(built):
    """the same identity where the chunked search differs most from the one-workgroup search: three chunks and a ragged tail,
    equal key distances inside chunks, across their boundaries and at the cut"""
    dev, ctx = _ctx()
    p, db, qs, _ = sq.chunk_case()
    _composition(ctx, dev, dict(p, dist_thresh=0.3), db, qs, "chunks")


def _assert_matches_reference(what, p, db, qs, got, prior):
    n_cases = 0
    for j in range(len(qs["desc"])):
        want = sq.ref_query(p, db["desc"], db["rk"], db["pos"], db["dist"], qs["desc"][j], qs["rk"][j], qs["pos"][j] if prior else None,
                            qs["dist"][j] if prior else None)
        assert not want["ties"], (what, j, "the reference does not decide this case: choose another query")
        print(what, "query", j, "loop", got["loop"][j], want["loop"], "min_dist", got["min_dist"][j], want["min_dist"],
              "largest |cand_dist - ref|", np.nanmax(np.abs(got["cand_dist"][j] - want["cand_dist"])))
        assert got["loop"][j] == want["loop"], (what, j)
        assert np.array_equal(got["cand_id"][j], want["cand_id"]), (what, j, got["cand_id"][j], want["cand_id"])
        assert np.array_equal(_bits(got["cand_yaw"][j]), _bits(want["cand_yaw"])), (what, j)
        assert _bits(got["yaw"][j:j + 1])[0] == _bits(np.array([want["yaw"]], dtype=np.float32))[0], (what, j)
        for g, w in zip(list(got["cand_dist"][j]) + [got["min_dist"][j]], list(want["cand_dist"]) + [want["min_dist"]]):
            assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= REL * max(1.0, abs(w)), (what, j, g, w)
        n_cases += 1
    return n_cases


@pytest.mark.parametrize("name", sq.PARITY_SETS)
def test_query_matches_numpy_reference(built, name):
    """against tests/scancontext_ref.py on all n_db entries: loop id, candidate ids in rank order and argmin-derived yaws
    identical, distances to the detect tests' bound; with and without the odometry prior.  The databases hold no planted
    tie descriptor, and the reference reports no shift or sector-key tie for any candidate of any query (asserted: no case
    is dropped); equal TOTAL distances of duplicated descriptors remain and go to the first rank on both sides."""
    dev, ctx = _ctx()
    p, db, qs = sq.parity_case(name, True)
    n = 0
    for prior in (True, False):
        n += _assert_matches_reference(name, p, db, qs, _gpu_query(ctx, dev, p, db, qs, prior=prior), prior)
    assert n == 2 * sq.N_PARITY_QUERIES


@pytest.mark.parametrize("n_db", [0, 1])
def test_query_on_an_empty_and_a_one_node_database(built, n_db):
    dev, ctx = _ctx()
    p, db, qs = sq.parity_case("staged_max", True)
    small = {k: v[:n_db] for k, v in db.items()}
    got = _gpu_query(ctx, dev, p, small, qs)
    assert _assert_matches_reference("n_db %d" % n_db, p, small, qs, got, True) == sq.N_PARITY_QUERIES
    K = p["num_candidates"]
    if n_db == 0:
        assert (got["loop"] == -1).all() and (got["yaw"] == 0).all() and (got["min_dist"] == sq.BIG).all()
        assert (got["cand_id"] == -1).all() and (got["cand_yaw"] == 0).all() and (got["cand_dist"] == sq.BIG).all()
    else:
        assert (got["cand_id"][:, 0] == 0).all() and (got["cand_id"][:, 1:] == -1).all() and (got["cand_dist"][:, 1:] == sq.BIG).all() and K > 1


def test_chunk_boundaries_and_ties(built):
    """3 chunks + 17 entries (the chunk length read from the source), duplicate ring keys inside a chunk, on both sides of
    every boundary and in the tail: the candidate list equals the reference's np.lexsort((index, distance)) order on every
    rank -- for a query whose nearest all lie in the ragged tail, one whose nearest lie one per chunk, one whose equal
    distances straddle the boundaries, one inside a chunk, one of the crowd; and for a database shorter than the rank count."""
    dev, ctx = _ctx()
    p, db, qs, planted = sq.chunk_case()
    C, K = sq.chunk_length(), p["num_candidates"]
    assert len(db["desc"]) == 3 * C + 17
    got = _gpu_query(ctx, dev, p, db, qs)
    names = list(planted) + ["crowd"]
    for j, name in enumerate(names):
        want, d2 = sq.ref_candidates(p, db["rk"], qs["rk"][j])
        print(name, "candidates", got["cand_id"][j], "reference", want, "key distances", d2[want])
        assert len(want) == K and np.array_equal(got["cand_id"][j], want), (name, got["cand_id"][j], want)
        if name != "crowd":
            assert set(want) <= set(planted[name]) or name == "per_chunk"
    # the cases are what they were planted to be
    assert all(i >= 3 * C for i in got["cand_id"][names.index("tail")]) and got["cand_id"][names.index("tail")][-1] == planted["tail"][K - 1]
    assert [int(i) // C for i in got["cand_id"][names.index("per_chunk")][:4]] == [0, 1, 2, 3]
    assert list(got["cand_id"][names.index("boundary")]) == planted["boundary"][:K]
    assert list(got["cand_id"][names.index("inside")]) == planted["inside"][:K]
    tie_at_cut = 0
    for j in range(len(names)):
        want, d2 = sq.ref_candidates(dict(p, num_candidates=K + 1), db["rk"], qs["rk"][j])
        tie_at_cut += d2[want[K - 1]] == d2[want[K]]
    assert tie_at_cut >= 3
    # fewer entries than ranks
    short = {k: v[C - 2:C + 1] for k, v in db.items()}
    got = _gpu_query(ctx, dev, p, short, qs)
    for j in range(len(names)):
        want, _ = sq.ref_candidates(p, short["rk"], qs["rk"][j])
        assert len(want) == 3 and np.array_equal(got["cand_id"][j], list(want) + [-1] * (K - 3)), (j, got["cand_id"][j])
        assert (got["cand_dist"][j][3:] == sq.BIG).all() and (got["cand_yaw"][j][3:] == 0).all()


def test_non_finite_keys(built):
    """the NaN rule: database entries with a NaN key are never candidates, at a chunk's first and last slot too; a NaN query
    finds nothing; an infinite key distance ranks last"""
    dev, ctx = _ctx()
    p, db, qs, info = sq.nonfinite_case()
    C = sq.chunk_length()
    assert info["nan"] == [0, C - 1, C, len(db["desc"]) - 1] and np.isnan(db["rk"][info["nan"]]).any(axis=1).all()
    got = _gpu_query(ctx, dev, p, db, qs)
    K, nq = p["num_candidates"], info["nan_query"]

    def candidates_equal(what, base, got):
        for j in range(len(qs["desc"])):
            want, d2 = sq.ref_candidates(p, base["rk"], qs["rk"][j])
            print(what, "query", j, "candidates", got["cand_id"][j], "reference", want)
            assert np.array_equal(got["cand_id"][j], list(want) + [-1] * (K - len(want))), (what, j)

    candidates_equal("nonfinite", db, got)
    assert not np.isin(got["cand_id"], info["nan"]).any() and (got["cand_id"][:nq] >= 0).all()
    assert got["loop"][nq] == -1 and got["min_dist"][nq] == sq.BIG and got["yaw"][nq] == 0 and (got["cand_id"][nq] == -1).all()
    assert (got["cand_dist"][nq] == sq.BIG).all() and (got["cand_yaw"][nq] == 0).all()
    # five entries, two of them NaN, one infinite: the finite ones, then the infinite one, then nothing
    p, small, qs, info = sq.nonfinite_small_case()
    got = _gpu_query(ctx, dev, p, small, qs)
    candidates_equal("nonfinite, 5 entries", small, got)
    for j in range(nq):
        assert sorted(got["cand_id"][j][:2]) == info["finite"] and got["cand_id"][j][2] == info["inf"] and (got["cand_id"][j][3:] == -1).all(), got["cand_id"][j]
    assert (got["cand_id"][nq] == -1).all()


def test_no_prior_is_the_descriptor_distance_alone(built):
    """q_pos / q_dist NULL: every total distance equals, bit for bit, the one with the prior given and odom_weight = 0 (finite
    inputs); the database's odometry may then be NULL too"""
    dev, ctx = _ctx()
    p, db, qs = sq.parity_case("indoor_600", True)
    assert p["odom_weight"] > 0
    zero = _gpu_query(ctx, dev, dict(p, odom_weight=0.0), db, qs, prior=True)
    with_w = _gpu_query(ctx, dev, p, db, qs, prior=True)
    assert not np.array_equal(with_w["cand_dist"], zero["cand_dist"])     # (the prior does something when it is given)
    for kw in (dict(prior=False), dict(prior=False, db_odom=False)):
        got = _gpu_query(ctx, dev, p, db, qs, **kw)
        for k in got:
            assert np.array_equal(_bits(got[k]) if got[k].dtype.kind == "f" else got[k], _bits(zero[k]) if zero[k].dtype.kind == "f" else zero[k]), (kw, k)


def test_per_candidate_outputs_are_consistent(built):
    """the best is the first minimum of cand_dist over the present ranks; loop_id is that rank's id iff its distance is below
    dist_thresh; absent ranks hold -1 / 0 / 10000000"""
    dev, ctx = _ctx()
    n_checked = n_hit = n_miss = 0
    for case, kw in ((sq.parity_case("indoor_600", False), {}), (sq.parity_case("staged_max", False), dict(prior=False)), (sq.nonfinite_small_case()[:3], {})):
        p, db, qs = case
        got = _gpu_query(ctx, dev, p, db, qs, **kw)
        for j in range(len(qs["desc"])):
            cid, cd, cy = got["cand_id"][j], got["cand_dist"][j], got["cand_yaw"][j]
            present = cid >= 0
            n_p = int(present.sum())
            assert present[:n_p].all() and (cid[n_p:] == -1).all() and (cd[n_p:] == sq.BIG).all() and (cy[n_p:] == 0).all()
            best, best_d = -1, sq.BIG
            for r in range(n_p):
                if cd[r] < best_d:
                    best, best_d = r, cd[r]
            assert got["min_dist"][j] == best_d
            if best >= 0:
                assert got["yaw"][j] == cy[best]
                assert got["loop"][j] == (cid[best] if best_d < p["dist_thresh"] else -1)
            else:
                assert got["loop"][j] == -1 and got["yaw"][j] == 0
            n_hit += got["loop"][j] >= 0
            n_miss += got["loop"][j] < 0
            n_checked += 1
    assert n_checked >= 12 and n_hit >= 1 and n_miss >= 1


def test_refusals(built):
    """sizes beyond the kernels: RANDT_ERR_UNSUPPORTED with a message, the outputs still hold their sentinel; no queries: RANDT_OK,
    nothing launched"""
    dev, ctx = _ctx()
    p, db, qs = sq.parity_case("staged_max", True)
    for kw in (dict(num_candidates=33), dict(num_ring=65), dict(num_sector=129), dict(num_candidates=0)):
        got = None
        with pytest.raises(R.RandtError) as e:
            got = _gpu_query(ctx, dev, dict(p, **kw), db, qs)
        assert e.value.status == R._capi.ERR_UNSUPPORTED and "scan context" in str(e.value), kw
        assert got is None
    # _gpu_query's outputs are out of reach after the raise: the same refusal with the tensors in hand
    import torch

    outs = [torch.full((2,), FILL_I, dtype=torch.int32, device=dev), torch.full((2,), FILL_F, dtype=torch.float32, device=dev),
            torch.full((2,), FILL_F, dtype=torch.float64, device=dev), torch.full((2, 33), FILL_I, dtype=torch.int32, device=dev),
            torch.full((2, 33), FILL_F, dtype=torch.float32, device=dev), torch.full((2, 33), FILL_F, dtype=torch.float64, device=dev)]
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)
    args = [up(db[k]) for k in ("desc", "rk", "pos", "dist")] + [up(qs[k][:2]) for k in ("desc", "rk", "pos", "dist")]
    for kw in (dict(num_candidates=33), dict(num_ring=65), dict(num_sector=129)):
        with pytest.raises(R.RandtError) as e:
            host.sc_query_batch(ctx, host.sc_params(**dict(p, **kw)), *args, *outs)
        ctx.synchronize()
        assert e.value.status == R._capi.ERR_UNSUPPORTED
        assert all(bool((o == (FILL_I if o.dtype == torch.int32 else FILL_F)).all()) for o in outs), kw
    # n_queries = 0: nothing is launched, nothing is written
    host.sc_query_batch(ctx, host.sc_params(**p), *args[:4], *[a[:0] for a in args[4:]], outs[0][:0], outs[1][:0], outs[2][:0], *outs[3:])
    ctx.synchronize()
    assert all(bool((o == (FILL_I if o.dtype == torch.int32 else FILL_F)).all()) for o in outs)
    # the context stays usable
    got = _gpu_query(ctx, dev, p, db, qs)
    assert (got["cand_id"][:, 0] >= 0).all()


# ------------------------------------------------------------------------------------------------- the database handle
def _scans(n, seed0):
    world = synth.make_world()
    traj = synth.make_trajectory(3100, n, step=0.6)
    return traj, [synth.make_scan(world, traj[i], seed0 + i) for i in range(n)]


def test_database_handle_query_and_restore(built):
    """randt_sc_db_query leaves the size and a downloaded node unchanged and equals the batch entry on the handle's arrays; a
    database rebuilt node by node from randt_sc_db_download through randt_sc_db_append_node answers randt_sc_db_detect (all
    nodes) and randt_sc_db_query like the original, bit for bit"""
    import torch

    dev, ctx = _ctx()
    n_db, n_q = 24, 4
    traj, scans = _scans(n_db + n_q, 5200)
    kw = dict(max_radius=20.0, num_exclude_recent=4, dist_thresh=0.5)
    sp = host.sc_params(**kw)
    pos = traj[:, :2].astype(np.float64)
    dist = np.concatenate([[0.0], np.cumsum(np.hypot(*np.diff(pos, axis=0).T))])
    db = host.ScDatabase(ctx, sp, capacity=4)
    for i in range(n_db):
        assert db.append(scans[i], pos[i], dist[i]) == i
    nodes = [db.download(i) for i in range(n_db)]
    answers = {}
    for j in range(n_db, n_db + n_q):
        for prior in (False, True):
            answers[j, prior] = db.query(scans[j], pos[j] if prior else None, dist[j] if prior else None)
    assert len(db) == n_db
    for i, (d, rk, sk) in enumerate(nodes):
        d2, rk2, sk2 = db.download(i)
        assert np.array_equal(_bits(d), _bits(d2)) and np.array_equal(_bits(rk), _bits(rk2)) and np.array_equal(_bits(sk), _bits(sk2)), i
    assert sum(a[0] >= 0 for a in answers.values()) >= 1
    # the batch entry on the same arrays; the queries' descriptors from the make kernel
    p = dict(cases.params(dict(R=sp.num_ring, S=sp.num_sector, num_exclude_recent=4, num_candidates=sp.num_candidates, search_ratio=sp.search_ratio,
                               odom_weight=sp.odom_weight)), **kw)
    pts = torch.from_numpy(np.stack(scans[n_db:])).to(dev)
    q_desc = torch.zeros((n_q, sp.num_sector, sp.num_ring), dtype=torch.float64, device=dev)
    q_rk = torch.zeros((n_q, sp.num_ring), dtype=torch.float64, device=dev)
    q_sk = torch.zeros((n_q, sp.num_sector), dtype=torch.float64, device=dev)
    host.sc_make_batch(ctx, pts, sp, q_desc, q_rk, q_sk)
    ctx.synchronize()
    arrays = dict(desc=np.stack([n[0] for n in nodes]), rk=np.stack([n[1] for n in nodes]), pos=pos[:n_db], dist=dist[:n_db])
    qs = dict(desc=q_desc.cpu().numpy(), rk=q_rk.cpu().numpy(), pos=pos[n_db:], dist=dist[n_db:])
    for prior in (False, True):
        got = _gpu_query(ctx, dev, p, arrays, qs, prior=prior)
        for j in range(n_q):
            lid, yaw, md, cid, cyaw, cd = answers[n_db + j, prior]
            assert lid == got["loop"][j] and np.float32(yaw) == got["yaw"][j] and md == got["min_dist"][j], (j, prior)
            assert np.array_equal(cid, got["cand_id"][j]) and np.array_equal(_bits(cyaw), _bits(got["cand_yaw"][j])) and np.array_equal(_bits(cd), _bits(got["cand_dist"][j]))
    # restored from the downloads
    db2 = host.ScDatabase(ctx, sp, capacity=4)
    for i, (d, rk, sk) in enumerate(nodes):
        assert db2.append_node(d, rk, sk, pos[i], dist[i]) == i
    assert len(db2) == n_db
    assert [db2.detect(i) for i in range(n_db)] == [db.detect(i) for i in range(n_db)]
    for (j, prior), want in answers.items():
        got = db2.query(scans[j], pos[j] if prior else None, dist[j] if prior else None)
        assert got[:3] == want[:3] and all(np.array_equal(_bits(a) if a.dtype.kind == "f" else a, _bits(b) if b.dtype.kind == "f" else b) for a, b in zip(got[3:], want[3:]))
    db.close()
    db2.close()


# ------------------------------------------------------------------------------------------------- the SLAM layer
def test_relocalize_in_a_mapped_loop(built):
    """the synthetic loop of tests/test_gpu_slam.py (its world, trajectory and parameters) until a submap is finished; then a
    held-out scan next to an early keyframe is relocalised, and a scan from a region the map never saw is not"""
    import torch

    n_scans, per_lap, dt = 300, 160, 0.25
    world = synth.make_world()
    th = 2 * np.pi * np.arange(n_scans) / per_lap
    truth = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    loop_mp = R.default_matcher_params(gnc_steps=2)
    sc = dict(max_radius=20.0, dist_thresh=0.5)
    s = slam.Slam(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params(), scan_slots=160, submap_slots=16), mp, R.window_params(),
                  loop_mp, params=dict(submap_size_poses=40, submap_overlap=10), sc_params=sc, loop_closure_weight=40.0)
    i = 0
    while s.n_finished_submaps < 1 or i < 56:
        s.process_scan(torch.from_numpy(synth.make_scan(world, truth[i], 71000 + i)).cuda(), i * dt)
        s.detect_loop_closures()
        i += 1
        assert i < 120
    assert 0 in s.submaps and len(s.nodes) >= 8
    before = (len(s.nodes), [n.copy() for n in s.nodes], [(a, b) for a, b, _, _ in s.edges], len(s.b._sc), list(s.submap_idzs), dict(s.root_nodes))

    # a held-out scan: between the scans 8 and 9 of the drive, a little off the track, its own noise seed
    tq = 2 * np.pi * 8.5 / per_lap
    true3 = np.array([5.1 * np.cos(tq), 5.1 * np.sin(tq), tq + np.pi / 2 + 0.05])
    held = synth.make_scan(world, true3, 990001)
    res = s.relocalize(held)
    assert res is not None

    # the same steps by hand, through the backend
    b = s.b
    scan = b.build_scan(held)
    _, _, _, cid, cyaw, cd = b.sc_query(held)
    best = None
    guesses = {}
    for lid, yaw, d in zip(cid.tolist(), cyaw.tolist(), cd.tolist()):
        if lid < 0 or not d < b.sc_dist_thresh() or s.submap_idzs[lid] not in s.submaps:
            continue
        sub_i = s.submap_idzs[lid]
        root = s.nodes[s.root_nodes[sub_i]]
        guess = odometry._se2_mul4(odometry._se2_mul4(odometry._se2_inv4(root), s.nodes[lid]), slam._pose4(-yaw, 0.0, 0.0))
        est, _ = b.register_pair(s.submaps[sub_i], scan, s.loop_mp, guess)
        cs = float(b.cs_divergence(s.submaps[sub_i], scan, est))
        guesses[lid] = odometry._se2_mul4(root, guess)
        if cs < s.max_cs and (best is None or cs < best[3]):
            best = (odometry._se2_mul4(root, est), lid, sub_i, cs, d)
    b.release_scan(scan)
    assert best is not None
    assert np.array_equal(_bits(res["pose"]), _bits(best[0])) and (res["node"], res["submap"]) == best[1:3]
    assert res["cs_divergence"] == best[3] and res["sc_distance"] == best[4]

    # the drive's frame is the first scan's pose
    origin_inv = synth.se2_inv3(truth[0])
    rel = synth.se2_mul3(origin_inv, true3)
    node3 = synth.pose4_to_pose3(s.nodes[res["node"]])
    assert np.hypot(node3[0] - rel[0], node3[1] - rel[1]) < sc["max_radius"]   # two scans can only match where they overlap
    got3, guess3 = synth.pose4_to_pose3(res["pose"]), synth.pose4_to_pose3(guesses[res["node"]])
    err, err_guess = np.hypot(got3[0] - rel[0], got3[1] - rel[1]), np.hypot(guess3[0] - rel[0], guess3[1] - rel[1])
    print("relocalised: node", res["node"], "cs", res["cs_divergence"], "sc distance", res["sc_distance"], "error", err, "error of the guess", err_guess)
    assert err < err_guess

    # a region the map never saw: another world
    other = synth.make_scan(synth.make_world(seed=4321), np.array([-13.0, 6.0, 2.0]), 990002)
    log_len, n_free = len(s.loop_log), len(s.b.free_scans)
    assert s.relocalize(other) is None
    after = (len(s.nodes), s.nodes, [(a, b) for a, b, _, _ in s.edges], len(s.b._sc), list(s.submap_idzs), dict(s.root_nodes))
    assert after[0] == before[0] and all(np.array_equal(x, y) for x, y in zip(after[1], before[1])) and after[2:] == before[2:]
    assert len(s.loop_log) == log_len and len(s.b.free_scans) == n_free
