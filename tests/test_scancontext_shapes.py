"""Scan Context at the database sizes and shapes the other tests never run (tests/scancontext_cases.py): beyond one
workgroup's stride of the candidate search, both column-shift searches, staged and unstaged descriptors, more than 64
sectors, empty sectors and all-zero descriptors, exact ties at every "first one wins", the bookkeeping of k_sc_make at
its edges, and non-finite keys.
CPU part: the oracle against a second restatement in numpy (tests/scancontext_ref.py), and the conditions that make the
inputs decidable (margins, planted ties, which branch a configuration reaches).  -m gpu part: the kernels against the oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
import scancontext_cases as cases
import scancontext_ref as ref
from randt_slam_amd import host, synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
REL = 1e-12          # the bound test_scancontext.py holds between the oracle and the kernels


def _close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


# ------------------------------------------------------------------------------------------------- CPU
@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """Runs the oracle and the numpy restatement over a set's queries ONCE (both are asserted equal here) and returns what
    the tests below count: margins and ties."""
    cs = cases.make_set(name) if name != "nonfinite" else cases.make_nonfinite_set()
    p, sp = cs["p"], cases.oracle_params(cs["p"])
    desc, rk, pos, dist = cs["desc"], cs["rk"], cs["pos"], cs["dist"]
    K = p["num_candidates"]
    st = dict(hits=0, sentinel=0, zero_dist=0, tie_ring=0, tie_ring_at_cut=0, tie_vkey=0, tie_shift=0, tie_pick=0, tie_vkey_won=0, tie_shift_won=0, short=0,
              min_gap=np.inf, min_thresh_margin=np.inf, sentinel_queries=[], max_n_search=0)
    o_lid, o_yaw, o_md = cases.oracle_detect(cs)
    for j, q in enumerate(int(v) for v in cs["queries"]):
        det = {}
        lid, yaw, md = ref.detect(p, desc, rk, pos, dist, q, det)
        assert o_lid[j] == lid and o_yaw[j] == yaw and _close(o_md[j], md), (name, q, (o_lid[j], o_yaw[j], o_md[j]), (lid, yaw, md))
        if not det:                                                        # the early return
            assert o_lid[j] == -1 and o_yaw[j] == 0 and o_md[j] == cases.BIG
            continue
        cand, d2 = det["candidates"], det["d2"]
        st["max_n_search"] = max(st["max_n_search"], len(d2))
        st["short"] += len(cand) < K
        # the oracle's distance to every candidate of the restatement: same shift, same value
        o_tot = []
        for c, t, sub in zip(cand, det["totals"], det["per_candidate"]):
            od, osh = po.sc_distance(sp, desc[q], desc[c], pos[q], pos[c], dist[q], dist[c])
            rd, rsh = t, sub["shift"]
            assert osh == rsh and _close(od, rd), (name, q, int(c), (od, osh), (rd, rsh))
            o_tot.append(od)
            st["tie_vkey"] += sub["vkey_tie"]
            st["tie_shift"] += sub["shift_tie"]
        # the conditions that make the answer decidable, on both sides
        for tot in (np.array(o_tot), det["totals"]):
            if len(tot) == 0:
                continue
            s = np.sort(tot)
            best = min(s[0], cases.BIG)
            if len(s) > 1 and s[0] < cases.BIG:
                gap = s[1] - s[0]
                assert gap == 0 or gap >= MARGIN, (name, q, gap)
                if gap > 0:
                    st["min_gap"] = min(st["min_gap"], gap)
            assert abs(best - p["dist_thresh"]) >= MARGIN, (name, q, best)
            st["min_thresh_margin"] = min(st["min_thresh_margin"], abs(best - p["dist_thresh"]))
        o_tot = np.array(o_tot)
        if len(o_tot) > 1 and o_tot.min() < cases.BIG:
            st["tie_pick"] += int((o_tot == o_tot.min()).sum() > 1)
        if len(o_tot) and o_tot.min() < cases.BIG:                         # ties that decided the ANSWER: in the winning candidate
            won = det["per_candidate"][int(np.argmin(o_tot))]
            st["tie_vkey_won"] += won["vkey_tie"]
            st["tie_shift_won"] += won["shift_tie"]
        # two equal key distances among the taken candidates, or between the last taken and the first left out
        sd = np.sort(d2[d2 >= 0])
        head = sd[: K + 1]
        st["tie_ring"] += bool(len(head) > 1 and (np.diff(head) == 0).any())
        st["tie_ring_at_cut"] += bool(len(sd) > K and sd[K - 1] == sd[K])
        st["hits"] += o_lid[j] >= 0
        st["zero_dist"] += o_md[j] == 0
        if o_md[j] == cases.BIG:
            st["sentinel"] += 1
            st["sentinel_queries"].append(q)
    return st


@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_oracle_matches_numpy_restatement(name):
    """pyoracle.sc_detect and pyoracle.sc_distance against tests/scancontext_ref.py on every query (candidate) of the set:
    loop id, yaw and shift equal, distances to 1e-12; per query the best two candidate distances are equal or >= 1e-9
    apart and the best one is >= 1e-9 from dist_thresh (asserted in _evaluate, on both sides)."""
    cs = cases.make_set(name)
    st = _evaluate(name)
    print(name, {k: v for k, v in st.items() if k != "sentinel_queries"})
    assert st["hits"] >= 1 and st["min_gap"] >= MARGIN and st["min_thresh_margin"] >= MARGIN
    # the planted nodes end where they were planted to: no column counts at any shift of the search space
    want = {cs["planted"][k] for k in ("zero_query", "zero_query_2", "pair_query") if k in cs["planted"]}
    assert want <= set(st["sentinel_queries"]) and st["sentinel"] >= len(want) >= 2
    assert st["tie_shift"] >= 1 and st["tie_vkey"] >= 1                   # the planted periodic descriptor
    if name == "tiny_4x8":
        assert st["short"] >= 1                                            # 2, 3 and 4 searchable entries for 3 ranks


def test_ties_occur_at_all_four_levels():
    """exact ties at the four "first one wins": ring-key distance (also across the cut between the last candidate taken and
    the first left out), sector-key shift, column shift, candidate pick.  The candidate-pick ties and the exact-zero
    distances are counted on the oracle's own values; the oracle's ABI does not hand out its key distances or per-shift
    values, so those three are counted on the restatement's, at queries where the oracle's answer was asserted equal --
    over every candidate (tie_vkey, tie_shift) and in the candidate that won the query (tie_*_won: the tie decided the yaw)."""
    tot = {k: 0 for k in ("tie_ring", "tie_ring_at_cut", "tie_vkey", "tie_shift", "tie_vkey_won", "tie_shift_won", "tie_pick", "zero_dist",
                          "sentinel")}
    for name in cases.CONFIGS:
        if cases.CONFIGS[name]["odom_weight"] == 0:                        # (the exp() term may split a planted tie)
            st = _evaluate(name)
            for k in tot:
                tot[k] += st[k]
    print(tot)
    assert all(v >= 1 for v in tot.values()), tot


def test_configurations_reach_the_kernel_branches():
    """both values of spread_shifts and of staged, n_search beyond two strides, more sectors than a wavefront has lanes --
    from the constants parsed out of scancontext.hip, not from a copy of them"""
    c = cases.kernel_constants()
    b = {name: cases.branches(cfg) for name, cfg in cases.CONFIGS.items()}
    for name, cfg in cases.CONFIGS.items():
        assert cfg["R"] <= c["SC_MAX_RING"] and cfg["S"] <= c["SC_MAX_SECTOR"] and 1 <= cfg["num_candidates"] <= c["SC_MAX_CAND"]
    assert not b["fallback_700"]["spread"] and b["fallback_700"]["terms"] > c["SC_TERM_CAP"] and b["fallback_700"]["n_shift"] <= 128
    assert b["fallback_700"]["n_search_max"] > 2 * c["SC_BLOCK"] and b["fallback_700"]["knn_trips"] >= 3
    assert _evaluate("fallback_700")["max_n_search"] > 2 * c["SC_BLOCK"]            # ... and a query that far back is in the set
    assert cases.CONFIGS["fallback_700"]["num_candidates"] == c["SC_MAX_CAND"] and b["fallback_700"]["beyond_first_wave"]
    assert b["unstaged_300"]["spread"] and not b["unstaged_300"]["staged"] and b["unstaged_300"]["n_search_max"] > c["SC_BLOCK"]
    assert b["staged_max"]["staged"] and b["staged_max"]["spread"]
    # the largest staged launch: one more ring (61 x 128) no longer fits, and 60 x 128 is within one ring (2 KB) of the rule's limit
    assert not b["unstaged_min"]["staged"] and b["unstaged_min"]["spread"]
    assert c["lds_limit"] - b["staged_max"]["staged_lds"] - c["staged_slack"] < 2 * 8 * 128
    assert b["spread_3968"]["spread"] and b["spread_3968"]["terms"] <= c["SC_TERM_CAP"] < b["fallback_4224"]["terms"]
    assert not b["fallback_4224"]["spread"] and b["fallback_4224"]["n_shift"] <= 128     # (refused by the term cap alone)
    assert not b["tiny_4x8"]["spread"] and b["tiny_4x8"]["n_shift"] > 8                  # duplicates in the search space
    assert b["indoor_600"]["spread"] and b["indoor_600"]["staged"] and b["indoor_600"]["n_search_max"] > 2 * c["SC_BLOCK"]
    assert {v["spread"] for v in b.values()} == {True, False} == {v["staged"] for v in b.values()}


def test_non_finite_keys_on_the_cpu():
    """A database entry whose float key distance is not >= 0 is never a candidate; with none left the remaining ranks are
    absent; a +inf distance IS >= 0 and ranks last.  Oracle and restatement agree on a database with two NaN nodes and one
    node with an infinite bin: a NaN node never wins, the infinite node wins the query it is a copy of."""
    cs = cases.make_nonfinite_set()
    st = _evaluate("nonfinite")
    o_lid, _, o_md = cases.oracle_detect(cs)
    q = list(cs["queries"])
    assert o_lid[q.index(30)] == -1 and o_md[q.index(30)] == cases.BIG             # the NaN node as a query: no candidate at all
    assert not set(o_lid) & {2, 30} and np.isfinite(o_md).all()
    # query 17 searches nodes 0, 1, 2: one finite distance, +inf (node 1, its copy but for an infinite bin in a sector the
    # query leaves empty), NaN -- two candidates for ten ranks, and the infinite one is the answer
    cand, d2 = ref.candidates(cs["p"], cs["rk"], 17)
    assert list(cand) == [0, 1] and np.isfinite(d2[0]) and np.isposinf(d2[1]) and np.isnan(d2[2])
    assert o_lid[q.index(17)] == 1 and o_md[q.index(17)] == 0.0
    assert 1 in ref.candidates(cs["p"], cs["rk"], 24)[0] and 1 not in ref.candidates(cs["p"], cs["rk"], 45)[0]
    assert st["short"] >= 3 and st["hits"] >= 1                                    # 17, 24 (9 valid entries for 10 ranks), 30


def test_oracle_non_finite_keys_under_sanitizers(tmp_path):
    """orc_sc_detect on a database with a NaN key, in a stand-alone program built with ASan + UBSan (before the rule the
    oracle wrote d2[-1])."""
    exe = str(tmp_path / "sc_nan_keys")
    subprocess.check_call(["gcc", "-O0", "-g", "-std=c99", "-ffp-contract=off", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "sc_nan_keys.c"), os.path.join(ROOT, "oracle", "randt_oracle.c"), "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    if "LeakSanitizer has encountered a fatal error" in r.stderr:          # (no ptrace here: everything but the leak check)
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------- GPU
def _ctx():
    import torch

    return torch.device("cuda:0"), R.Context(0, torch.cuda.current_stream().cuda_stream)


def _gpu_detect(ctx, dev, cs, queries, want_min_dist=True, untouched=False):
    """randt_sc_detect_batch_dev over a set; queries None = every node in order (no query_ids array).  untouched: for a call
    that is expected to be refused -- the outputs must still hold what they were filled with"""
    import torch

    sp = host.sc_params(**cs["p"])
    n = len(cs["desc"]) if queries is None else len(queries)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)                  # (a copy: the sets are read-only and shared)
    loop = torch.full((n,), -7, dtype=torch.int32, device=dev)
    yaw = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    md = torch.full((n,), -7.0, dtype=torch.float64, device=dev) if want_min_dist else None
    try:
        host.sc_detect_batch(ctx, sp, up(cs["desc"]), up(cs["rk"]), up(cs["pos"]), up(cs["dist"]), None if queries is None else up(queries),
                             loop, yaw, md)
    finally:
        ctx.synchronize()
        if untouched:
            assert bool((loop == -7).all()) and bool((yaw == -7.0).all()) and bool((md == -7.0).all())
    return loop.cpu().numpy(), yaw.cpu().numpy(), md.cpu().numpy() if want_min_dist else None


def _assert_detect_equal(name, queries, got, want, bit_equal):
    (loop, yaw, md), (o_lid, o_yaw, o_md) = got, want
    worst = 0.0
    for j, q in enumerate(queries):
        assert loop[j] == o_lid[j], (name, int(q), loop[j], o_lid[j])
        assert yaw[j] == o_yaw[j], (name, int(q), yaw[j], o_yaw[j])
        assert abs(md[j] - o_md[j]) <= REL * max(1.0, abs(o_md[j])), (name, int(q), md[j], o_md[j])
        worst = max(worst, abs(md[j] - o_md[j]))
    print(name, "queries", len(queries), "largest |min_dist - oracle|", worst)
    if bit_equal:
        assert np.array_equal(md, o_md), (name, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CONFIGS))
def test_hip_detect_matches_oracle_at_database_shapes(built, name):
    """k_sc_knn / k_sc_detect / k_sc_pick against the oracle on the synthetic databases: loop id and yaw equal, the minimal
    distance to 1e-12 -- and BIT-EQUAL where odom_weight = 0 leaves no exp() in it: every remaining operation (+, *, /,
    sqrt in double, in the oracle's order) is correctly rounded on both sides.  Measured on an MI355X: bit-equal in all six
    such sets; 8.9e-16 (unstaged_300) and 0 (indoor_600) with the default odometry weight."""
    dev, ctx = _ctx()
    cs = cases.make_set(name)
    c = cases.kernel_constants()
    import torch

    # the device's own LDS limit decides `staged`: the configuration must reach the branch it is named for HERE
    lds = torch.cuda.get_device_properties(0).shared_memory_per_block
    assert cases.branches(cs["cfg"], lds)["staged"] == cases.branches(cs["cfg"])["staged"], (lds, c["lds_limit"])
    got = _gpu_detect(ctx, dev, cs, cs["queries"])
    _assert_detect_equal(name, cs["queries"], got, cases.oracle_detect(cs), bit_equal=cs["cfg"]["odom_weight"] == 0)
    q = list(cs["queries"])                                               # the planted queries reached the kernels, not the early return
    for k in ("zero_query", "zero_query_2", "pair_query"):
        if k in cs["planted"]:
            j = q.index(cs["planted"][k])
            assert cs["planted"][k] > cs["cfg"]["num_exclude_recent"] and got[2][j] == cases.BIG and got[0][j] == -1, (name, k)
    assert (got[0] >= 0).sum() >= 1


@pytest.mark.gpu
def test_hip_detect_without_query_ids(built):
    """query_ids = NULL: query q is node q; and without the min_dist output"""
    dev, ctx = _ctx()
    cs = cases.make_set("spread_3968")
    every = np.arange(len(cs["desc"]), dtype=np.int32)
    want = cases.oracle_detect(cs, every)
    _assert_detect_equal("spread_3968, no query_ids", every, _gpu_detect(ctx, dev, cs, None), want, bit_equal=True)
    loop, yaw, _ = _gpu_detect(ctx, dev, cs, None, want_min_dist=False)
    assert np.array_equal(loop, want[0]) and np.array_equal(yaw, want[1])


def _ring_sector_point(sp, ring, sect, rng):
    """a point well inside bin (ring, sect) (0-based)"""
    r = (ring + rng.uniform(0.3, 0.7)) * sp["max_radius"] / sp["num_ring"]
    a = np.deg2rad((sect + rng.uniform(0.3, 0.7)) * 360.0 / sp["num_sector"])
    return r * np.cos(a), r * np.sin(a)


def _make_edge_scans(sp, pitch, rng):
    """the ragged batch of the k_sc_make edge test: (points [B][pitch][8] PCL layout, counts [B])"""
    Rn, Sn, rad = sp["num_ring"], sp["num_sector"], sp["max_radius"]
    scans, counts = [], []

    def add(xy):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        m = len(xy)
        p = np.zeros((pitch, 8), dtype=F)
        p[:, :2] = 1.0                                                     # rows beyond the count: in range and loud, never to be read
        p[:, 4] = 1e6
        p[:m, :2] = xy
        p[:m, 4] = rng.uniform(5, 95, m)
        p[:m, 2] = rng.uniform(-1, 1, m)                                   # a height the descriptor ignores
        scans.append(p)
        counts.append(m)

    rr, ang = rng.uniform(0.2, rad * 1.05, pitch), rng.uniform(0, 2 * np.pi, pitch)  # (some beyond the rim)
    full = np.stack([rr * np.cos(ang), rr * np.sin(ang)], 1)
    for n in (0, 1, 63, 64, 65, pitch):                                    # below / at / above one wavefront, and the whole pitch
        add(full[:n])
    b = (Sn // 3) * Rn + Rn // 2                                           # every point in ONE bin, input order: the longest chain
    add([_ring_sector_point(sp, b % Rn, b // Rn, rng) for _ in range(pitch)])
    far = rng.uniform(rad * 1.01, rad * 3, pitch)                          # nothing within max_radius: all-zero outputs
    add(np.stack([far * np.cos(ang), far * np.sin(ang)], 1))
    b1, b2 = 1, 1 + 4 * (Rn // 4 if Rn >= 8 else 1) + 4 * Rn * (Sn // 8)    # two bins, indices congruent mod 4: one wavefront's share
    assert b1 % 4 == b2 % 4 and b1 != b2 and b2 < Rn * Sn
    add([_ring_sector_point(sp, (b1 if i % 2 == 0 else b2) % Rn, (b1 if i % 2 == 0 else b2) // Rn, rng) for i in range(pitch)])
    # exactly on ring and sector boundaries, on the axes, at the origin, on the rim
    edge = [(0.0, 0.0), (rad, 0.0), (0.0, rad), (-rad, 0.0), (0.0, -rad), (-0.0, 1.0), (1.0, -0.0), (-0.0, -1.0)]
    for k in range(1, Rn + 1):
        edge += [(k * rad / Rn, 0.0), (0.0, k * rad / Rn), (-(k * rad / Rn), 0.0), (0.0, -(k * rad / Rn))]
    for s in range(Sn):
        a = np.deg2rad(s * 360.0 / Sn)
        edge += [(0.5 * rad * np.cos(a), 0.5 * rad * np.sin(a)), (float(F(rad)) * np.cos(a), float(F(rad)) * np.sin(a))]
    assert len(edge) <= pitch
    add(edge)
    return np.stack(scans), np.array(counts, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 8), (64, 128), (20, 45)])
def test_hip_sc_make_edges(built, shape):
    """k_sc_make's bookkeeping: an odd pitch (the sorted values start at a rounded-up offset), counts 0 / 1 / 63 / 64 / 65 /
    pitch, every point in one bin, every point out of range, two bins of one wavefront's share, points ON the ring and
    sector boundaries and the axes; fewer bins than threads (32) and 8192 of them; PCL stride 8, intensity at 4.
    Descriptors, ring keys and sector keys bit-equal to the oracle."""
    import torch

    dev, ctx = _ctx()
    kw = dict(num_ring=shape[0], num_sector=shape[1], max_radius=20.0, intensity_factor=0.04)
    sp_o, sp = cases.oracle_params({**cases.params(dict(R=shape[0], S=shape[1], num_exclude_recent=15, num_candidates=10, search_ratio=0.1,
                                                        odom_weight=0.2)), **kw}), host.sc_params(**kw)
    pitch = 1999
    pts, n_pts = _make_edge_scans(kw, pitch, np.random.default_rng(shape[0]))
    B, nb = len(pts), shape[0] * shape[1]
    d_desc = torch.full((B, shape[1], shape[0]), 7.0, dtype=torch.float64, device=dev)
    d_rk = torch.full((B, shape[0]), 7.0, dtype=torch.float64, device=dev)
    d_sk = torch.full((B, shape[1]), 7.0, dtype=torch.float64, device=dev)
    host.sc_make_batch(ctx, torch.from_numpy(pts).to(dev), sp, d_desc, d_rk, d_sk, n_points=torch.from_numpy(n_pts).to(dev))
    ctx.synchronize()
    g_desc, g_rk, g_sk = d_desc.cpu().numpy(), d_rk.cpu().numpy(), d_sk.cpu().numpy()
    for i in range(B):
        d, rk, sk = po.sc_make(pts[i, :n_pts[i]], sp_o)
        assert np.array_equal(g_desc[i], d) and np.array_equal(g_rk[i], rk) and np.array_equal(g_sk[i], sk), (shape, i, int(n_pts[i]))
    assert not g_desc[0].any() and not g_desc[7].any() and not g_rk[7].any()      # n = 0, and everything beyond max_radius
    assert np.count_nonzero(g_desc[6]) == 1 and np.count_nonzero(g_desc[8]) == 2  # one bin / two bins
    assert np.count_nonzero(g_desc[5]) > min(nb, 200) // 2
    # without the count array every scan holds `pitch` points
    host.sc_make_batch(ctx, torch.from_numpy(pts[5:7]).to(dev), sp, d_desc[:2], d_rk[:2], d_sk[:2])
    ctx.synchronize()
    assert np.array_equal(d_desc[:2].cpu().numpy(), g_desc[5:7]) and np.array_equal(d_sk[:2].cpu().numpy(), g_sk[5:7])


@pytest.mark.gpu
def test_hip_scan_context_refusals(built):
    """sizes beyond the kernels are status codes, not launches: RANDT_ERR_UNSUPPORTED, outputs untouched"""
    import torch

    dev, ctx = _ctx()
    pts = torch.zeros((2, 4000, 4), dtype=torch.float32, device=dev)
    pts[:, :, 0] = 3.0
    pts[:, :, 3] = 50.0

    def make_refused(pitch, **kw):
        sp = host.sc_params(**kw)
        out = [torch.full((2, sp.num_sector, sp.num_ring), 7.0, dtype=torch.float64, device=dev),
               torch.full((2, sp.num_ring), 7.0, dtype=torch.float64, device=dev), torch.full((2, sp.num_sector), 7.0, dtype=torch.float64, device=dev)]
        with pytest.raises(R.RandtError) as e:
            host.sc_make_batch(ctx, pts[:, :pitch].contiguous(), sp, *out)
        ctx.synchronize()
        assert e.value.status == R._capi.ERR_UNSUPPORTED and all(bool((o == 7.0).all()) for o in out), kw

    make_refused(2000, num_ring=65, num_sector=128)
    make_refused(2000, num_ring=64, num_sector=129)
    make_refused(4000, num_ring=64, num_sector=128)                        # 48 KB of points + 128 KB of bins: beyond the LDS
    cs = cases.make_set("tiny_4x8")
    for kw in (dict(num_candidates=0), dict(num_candidates=33), dict(num_ring=65), dict(num_sector=129)):
        with pytest.raises(R.RandtError) as e:
            _gpu_detect(ctx, dev, dict(cs, p=dict(cs["p"], **kw)), cs["queries"], untouched=True)
        assert e.value.status == R._capi.ERR_UNSUPPORTED, kw
    # the context stays usable, and a 64 x 128 descriptor at a pitch that fits is served
    sp = host.sc_params(num_ring=64, num_sector=128)
    out = [torch.zeros((2, 128, 64), dtype=torch.float64, device=dev), torch.zeros((2, 64), dtype=torch.float64, device=dev),
           torch.zeros((2, 128), dtype=torch.float64, device=dev)]
    host.sc_make_batch(ctx, pts[:, :2000].contiguous(), sp, *out)
    ctx.synchronize()
    assert np.count_nonzero(out[0].cpu().numpy()) == 2


@functools.lru_cache(maxsize=None)
def _stationary_drive():
    """300 keyframes of 200 points from the synthetic world: a circle driven 2.3 times round (so places are revisited),
    standing still for nodes 200 .. 204 (the same scan five times)"""
    world = synth.make_world()
    th = 2 * np.pi * np.arange(300) / 130
    traj = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    scans = [synth.make_scan(world, traj[i], 30000 + i)[3::10].copy() for i in range(300)]
    for i in range(201, 205):
        traj[i], scans[i] = traj[200], scans[200]
    pos = traj[:, :2].copy()
    dist = np.cumsum(np.full(300, 0.25))                                   # (strictly increasing through the stop, like a clock)
    return scans, pos, dist


@pytest.mark.gpu
def test_hip_scan_context_database_beyond_one_stride(built):
    """randt_sc_db_* with more searchable nodes than one workgroup's stride, identical keyframes in a row and a dozen
    re-allocations from a capacity of 8"""
    dev, ctx = _ctx()
    kw = dict(max_radius=20.0, dist_thresh=0.5)
    sp_o, sp = cases.oracle_params({**cases.params(cases.CONFIGS["indoor_600"]), **kw}), host.sc_params(**kw)
    scans, pos, dist = _stationary_drive()
    db = host.ScDatabase(ctx, sp, capacity=8)
    descs, rks, sks = [], [], []
    for i, s in enumerate(scans):
        assert db.append(s, pos[i], dist[i]) == i
        d, rk, sk = po.sc_make(s, sp_o)
        descs.append(d)
        rks.append(rk)
        sks.append(sk)
    assert len(db) == 300 and 300 - sp.num_exclude_recent > cases.kernel_constants()["SC_BLOCK"]
    descs, rks = np.stack(descs), np.stack(rks)
    assert np.array_equal(descs[200], descs[204])
    for i in (0, 202, 299):
        d, rk, sk = db.download(i)
        assert np.array_equal(d, descs[i]) and np.array_equal(rk, rks[i]) and np.array_equal(sk, sks[i])
    hits = 0
    for i in (15, 16, 150, 200, 201, 202, 203, 204, 219, 220, 280, 299):
        lid, yaw, md = db.detect(i)
        olid, oyaw, omd = po.sc_detect(sp_o, descs, rks, pos, dist, i)
        assert lid == olid and yaw == np.float32(oyaw) and abs(md - omd) <= REL * max(1.0, abs(omd)), (i, lid, olid, md, omd)
        hits += lid >= 0
    assert hits >= 1
    db.close()


@pytest.mark.gpu
def test_hip_non_finite_keys(built):
    """The rule of test_non_finite_keys_on_the_cpu on the device: a NaN key distance is never a candidate, ranks without a
    candidate are absent (k_sc_knn leaves -1 and retires nothing), the NaN node as a query finds nothing; an infinite key
    distance is taken (last in rank), and the node that holds it wins query 17."""
    dev, ctx = _ctx()
    cs = cases.make_nonfinite_set()
    want = cases.oracle_detect(cs)
    got = _gpu_detect(ctx, dev, cs, cs["queries"])
    _assert_detect_equal("nonfinite", cs["queries"], got, want, bit_equal=True)
    q = list(cs["queries"])
    assert got[0][q.index(30)] == -1 and got[2][q.index(30)] == cases.BIG and not set(got[0]) & {2, 30}
    assert got[0][q.index(17)] == 1 and got[2][q.index(17)] == 0.0
    # the context is healthy afterwards: the same call again, same answer
    again = _gpu_detect(ctx, dev, cs, cs["queries"])
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
