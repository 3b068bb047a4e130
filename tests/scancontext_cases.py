"""Synthetic Scan Context databases for the CPU and GPU tests of tests/test_scancontext_shapes.py (test infrastructure,
numpy only -- the oracle is imported lazily, by the functions that run it).

The detect entry takes descriptors and ring keys directly, so a database needs no scans: a few dozen "places" (sparse
integer-valued S x R arrays, several sectors entirely empty); four nodes in five are a place rolled by a random column shift
with a sprinkle of small integer perturbations, the rest are exact copies of a place in its one "standing still" heading --
identical keyframes, which plant the exact ties at the ring-key and candidate-pick level.  Planted on top: all-zero
descriptors, a pair whose non-empty sectors never meet, and a descriptor periodic in the sectors (ties between shifts).
Integer values keep every column dot product and squared norm exact, so a planted tie is a tie on every side.

branches() restates the launch decisions of csrc/scancontext.hip from the constants it PARSES out of that file, so that a
later change of a constant makes the coverage test say which branch is no longer reached."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "randt-slam_amd", "csrc")
BIG = 10000000.0

#        name              R   S    search_ratio  candidates  exclude  n_db  odom_weight  planted pair
CONFIGS = {
    "fallback_700": dict(R=16, S=128, search_ratio=0.3, num_candidates=32, num_exclude_recent=30, n_db=700, odom_weight=0.0, pair=True),
    "unstaged_300": dict(R=64, S=128, search_ratio=0.1, num_candidates=10, num_exclude_recent=15, n_db=300, odom_weight=0.2, pair=True),
    "staged_max": dict(R=60, S=128, search_ratio=0.1, num_candidates=10, num_exclude_recent=15, n_db=40, odom_weight=0.0, pair=True),
    "unstaged_min": dict(R=61, S=128, search_ratio=0.1, num_candidates=10, num_exclude_recent=15, n_db=40, odom_weight=0.0, pair=True),
    "spread_3968": dict(R=20, S=128, search_ratio=0.234, num_candidates=10, num_exclude_recent=15, n_db=60, odom_weight=0.0, pair=True),
    "fallback_4224": dict(R=20, S=128, search_ratio=0.25, num_candidates=10, num_exclude_recent=15, n_db=60, odom_weight=0.0, pair=True),
    "tiny_4x8": dict(R=4, S=8, search_ratio=1.2, num_candidates=3, num_exclude_recent=2, n_db=40, odom_weight=0.0, pair=False),
    "indoor_600": dict(R=20, S=45, search_ratio=0.3, num_candidates=10, num_exclude_recent=15, n_db=600, odom_weight=0.2, pair=True),
}
DIST_THRESH = 0.3
N_PLACES = 24
PERIOD = {128: 8, 45: 5, 8: 2}      # sectors after which the planted periodic descriptor repeats


def params(cfg):
    """the randt_sc_params / orc_sc_params fields of a configuration (max_radius and intensity_factor only matter to sc_make)"""
    return dict(num_ring=cfg["R"], num_sector=cfg["S"], max_radius=15.0, num_exclude_recent=cfg["num_exclude_recent"],
                num_candidates=cfg["num_candidates"], search_ratio=cfg["search_ratio"], dist_thresh=DIST_THRESH, assumed_drift=0.05,
                odom_eps=1.2, odom_weight=cfg["odom_weight"], intensity_factor=0.04)


FIELDS = ("num_ring", "num_sector", "max_radius", "num_exclude_recent", "num_candidates", "search_ratio", "dist_thresh", "assumed_drift",
          "odom_eps", "odom_weight", "intensity_factor")


def oracle_params(p):
    import pyoracle as po

    return po.ScParams(*[p[k] for k in FIELDS])


# ------------------------------------------------------------------------------------------ the kernel's own formulas
@functools.lru_cache(maxsize=None)
def kernel_constants():
    src = open(os.path.join(CSRC, "scancontext.hip")).read()
    hdr = open(os.path.join(CSRC, "randt_internal.h")).read()

    def one(pattern, text, what):
        m = re.search(pattern, text)
        assert m, "scancontext.hip no longer states %s the way tests/scancontext_cases.py reads it: update branches()" % what
        return [int(g) for g in m.groups()]

    c = {}
    for name in ("SC_BLOCK", "SC_MAX_SECTOR", "SC_MAX_RING", "SC_MAX_CAND", "SC_TERM_CAP"):
        c[name] = one(r"#define %s (\d+)" % name, src, name)[0]
    a, b = one(r"int lds_limit = (\d+) \* (\d+);", hdr, "the default LDS limit")
    c["lds_limit"] = a * b
    a, b = one(r"staged = lds \+ (\d+) \* (\d+) <= \(size_t\)ctx->lds_limit", src, "the staging rule")
    c["staged_slack"] = a * b
    assert "spread_shifts = n_shift <= S && n_shift * S <= SC_TERM_CAP;" in src, "the spread rule of k_sc_detect changed: update branches()"
    assert "for (int i = tid; i < n_search; i += SC_BLOCK)" in src, "k_sc_knn no longer strides the database by SC_BLOCK: update branches()"
    return c


def branches(cfg, lds_limit=None):
    """which paths of launch_sc_detect / k_sc_knn / k_sc_detect a configuration takes"""
    c = kernel_constants()
    R, S = cfg["R"], cfg["S"]
    radius = int(np.floor(0.5 * cfg["search_ratio"] * S + 0.5))
    n_shift = 2 * radius + 1
    n_search_max = cfg["n_db"] - cfg["num_exclude_recent"]
    return dict(radius=radius, n_shift=n_shift, terms=n_shift * S,
                spread=n_shift <= S and n_shift * S <= c["SC_TERM_CAP"],
                staged=2 * 8 * R * S + c["staged_slack"] <= (lds_limit or c["lds_limit"]),
                staged_lds=2 * 8 * R * S,
                n_search_max=n_search_max, knn_trips=-(-n_search_max // c["SC_BLOCK"]),
                beyond_first_wave=S > 64)


# ------------------------------------------------------------------------------------------ databases
def keys_of(desc):
    """ring keys in sc_make's order: the left-to-right sum over the sectors, divided by S"""
    return np.add.accumulate(desc, axis=1)[:, -1, :] / desc.shape[1]


def _place(rng, S, R):
    p = np.where(rng.random((S, R)) < 0.3, rng.integers(1, 9, (S, R)), 0).astype(np.float64)
    empty = rng.choice(S, size=max(1, S // 6), replace=False)              # whole sectors a filtered scan leaves empty
    p[empty] = 0
    return p


@functools.lru_cache(maxsize=None)
def make_set(name):
    """dict: p (parameter fields), desc [n][S][R], rk [n][R], pos [n][2], dist [n], queries (int32), planted {role: node}"""
    cfg = CONFIGS[name]
    R, S, n_db, ex = cfg["R"], cfg["S"], cfg["n_db"], cfg["num_exclude_recent"]
    rng = np.random.default_rng(sorted(CONFIGS).index(name) + 100)
    places = [_place(rng, S, R) for _ in range(N_PLACES)]
    stand = rng.integers(S, size=N_PLACES)                                  # the heading in which a place is seen standing still
    desc = np.zeros((n_db, S, R))
    for i in range(n_db):
        k = rng.integers(N_PLACES)
        if rng.random() < 0.8:
            d = np.roll(places[k], int(rng.integers(S)), axis=0)
            filled, m = np.flatnonzero(d.any(axis=1)), max(3, (S * R) // 40)
            np.add.at(d, (rng.choice(filled, m), rng.integers(R, size=m)), rng.integers(1, 4, m))
        else:
            # an exact copy, heading included: identical keyframes tie EXACTLY.  (The same place unperturbed under another
            # heading would give the same cosine terms in another order -- sums one ulp apart, neither a tie nor a margin.)
            d = np.roll(places[k], int(stand[k]), axis=0)
        desc[i] = d
    planted = {}
    # an all-zero descriptor as a candidate (node 0) and as a query (two more: the second has the others at key distance 0)
    planted["zero_first"] = 0
    planted["zero_query"] = n_db // 2
    planted["zero_query_2"] = n_db // 2 + 3
    for k in ("zero_first", "zero_query", "zero_query_2"):
        desc[planted[k]] = 0
    if cfg["pair"]:
        # a pair whose non-empty sectors never meet: the query holds +2 in sector 0, its only searchable entries are the zero
        # node and two nodes that hold negative values in sector S / 2.  Aligning the sector keys AVOIDS the overlap (opposite
        # signs: (2 + 2)^2 > 2^2 + 2^2), every other shift ties, the first (0) wins and the search space 0 +- radius stays away
        # from S / 2: no column counts at any shift
        assert branches(cfg)["radius"] < S // 2
        planted["pair_a"], planted["pair_b"], planted["pair_query"] = 1, 2, ex + 2
        for k, v in (("pair_a", -2.0), ("pair_b", -3.0)):
            desc[planted[k]] = 0
            desc[planted[k], S // 2, :] = v
        desc[planted["pair_query"]] = 0
        desc[planted["pair_query"], 0, :] = 2.0
    # a descriptor that repeats every `period` sectors, twice: shifts one period apart give the same terms column by column,
    # an exact tie between two shifts of the search space (and between shifts of the sector keys)
    period = PERIOD[S]
    assert S % period == 0 and period <= 2 * branches(cfg)["radius"]
    block = np.where(rng.random((period, R)) < 0.5, rng.integers(1, 9, (period, R)), 0).astype(np.float64)
    block[0], block[1] = 0, np.arange(1, R + 1) % 8 + 1
    planted["periodic"], planted["periodic_query"] = 3, n_db // 2 + 5
    desc[planted["periodic"]] = desc[planted["periodic_query"]] = np.tile(block, (S // period, 1))
    rk = keys_of(desc)
    sigma = 0.15 if cfg["odom_weight"] else 0.4
    pos = np.cumsum(rng.normal(0, sigma, (n_db, 2)), axis=0)
    dist = np.cumsum(rng.uniform(0.3, 0.7, n_db))                           # strictly increasing
    q = set(range(0, n_db, max(1, n_db // 100)))
    q |= {ex, ex + 1, ex + 2, ex + 3, n_db - 1, n_db} | set(planted.values())
    queries = np.array(sorted(q), dtype=np.int32)
    for a in (desc, rk, pos, dist, queries):
        a.setflags(write=False)
    return dict(name=name, cfg=cfg, p=params(cfg), desc=desc, rk=rk, pos=pos, dist=dist, queries=queries, planted=planted)


@functools.lru_cache(maxsize=None)
def make_nonfinite_set():
    """the shipped indoor shape, 60 nodes, two of them with a NaN in one bin (and so in one ring key): node 2 among the first
    entries -- the queries just behind the exclusion window then have FEWER valid entries than ranks -- and node 30; and node 1
    with an INFINITE bin: a copy of node 17 with +inf in a sector node 17 leaves empty.  Its key distance to a finite query is
    +inf, which is >= 0: it is a candidate (last in rank) of the queries 16 .. 24, and for query 17 it must win with distance 0"""
    cfg = dict(R=20, S=45, search_ratio=0.3, num_candidates=10, num_exclude_recent=15, n_db=60, odom_weight=0.0, pair=False)
    rng = np.random.default_rng(77)
    places = [_place(rng, 45, 20) for _ in range(6)]
    desc = np.stack([np.roll(places[rng.integers(6)], int(rng.integers(45)), axis=0) for _ in range(60)])
    for node in (2, 30):
        desc[node, 5, 3] = np.nan
    desc[1] = desc[17]
    desc[1, np.flatnonzero(~desc[17].any(axis=1))[0], 4] = np.inf
    with np.errstate(invalid="ignore"):
        rk = keys_of(desc)
    assert np.isnan(rk[[2, 30], 3]).all() and np.isposinf(rk[1, 4]) and np.isfinite(np.delete(rk, [1, 2, 30], axis=0)).all()
    pos = np.cumsum(rng.normal(0, 0.4, (60, 2)), axis=0)
    dist = np.cumsum(rng.uniform(0.3, 0.7, 60))
    # 16: node 0 and the infinite node; 17: 3 entries, one NaN, one infinite (the winner); 24: 10 entries = the rank count, 9 valid; 25: 10 valid of 11; 30: the NaN node itself;
    # 45 ..: both NaN nodes searchable
    queries = np.array([16, 17, 20, 24, 25, 29, 30, 31, 44, 45, 46, 52, 59], dtype=np.int32)
    return dict(name="nonfinite", cfg=cfg, p=params(cfg), desc=desc, rk=rk, pos=pos, dist=dist, queries=queries, planted={"nan": (2, 30), "inf": 1, "inf_query": 17})


def oracle_detect(cs, queries=None):
    """pyoracle.sc_detect over the queries of a set: (loop ids, yaws as float32, minimal distances)"""
    import pyoracle as po

    sp = oracle_params(cs["p"])
    queries = cs["queries"] if queries is None else queries
    out = [po.sc_detect(sp, cs["desc"], cs["rk"], cs["pos"], cs["dist"], int(q)) for q in queries]
    return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float64))
