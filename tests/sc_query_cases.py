"""Inputs and the numpy reference for the Scan Context QUERY entry (randt_sc_query_batch_dev): a scan that is not a node
against every node of a database.  Test infrastructure, numpy only; built on tests/scancontext_cases.py (databases) and
tests/scancontext_ref.py (the restatement of SCManager), both imported, neither edited."""
import functools
import os
import re

import numpy as np

import scancontext_cases as cases
import scancontext_ref as ref

BIG = ref.BIG


@functools.lru_cache(maxsize=None)
def chunk_length():
    """SCQ_CHUNK, parsed out of csrc/scancontext_query.hip like scancontext_cases.kernel_constants parses the others"""
    src = open(os.path.join(cases.CSRC, "scancontext_query.hip")).read()
    m = re.search(r"#define SCQ_CHUNK (\d+)", src)
    assert m, "scancontext_query.hip no longer states SCQ_CHUNK the way tests/sc_query_cases.py reads it"
    assert "for (int j = tid; j < len; j += SC_BLOCK)" in src, "k_scq_chunk no longer strides its chunk by SC_BLOCK"
    return int(m.group(1))


def yaw_of(shift, S):
    return np.float32(float(np.float32(shift * (360.0 / S))) * np.pi / 180.0)     # scancontext_ref.detect's last line


def ref_candidates(p, rk, q_rk):
    """the num_candidates nearest of ALL entries in (float key distance, index) order, NaN rule applied; and the distances"""
    n = len(rk)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = ref.key_distances(np.concatenate([np.asarray(rk), np.asarray(q_rk)[None]]), n, n)
        order = np.lexsort((np.arange(n), d2))
        order = order[d2[order] >= 0]
    return order[: p["num_candidates"]], d2


def ref_query(p, desc, rk, pos, dist, q_desc, q_rk, q_pos=None, q_dist=None):
    """What randt_sc_query_batch_dev must return for one query, from scancontext_ref: dict(loop, yaw, min_dist, cand_id,
    cand_yaw, cand_dist [num_candidates each, absent ranks -1 / 0 / BIG], ties = some candidate's shift or sector-key tie)."""
    K, S = p["num_candidates"], p["num_sector"]
    prior = q_pos is not None and q_dist is not None
    pp = p if prior else dict(p, odom_weight=0.0)                          # no prior: the descriptor distance alone
    cand, _ = ref_candidates(p, rk, q_rk)
    out = dict(cand_id=np.full(K, -1, dtype=np.int32), cand_yaw=np.zeros(K, dtype=np.float32), cand_dist=np.full(K, BIG), ties=False)
    min_d, nn_align, nn_idx = BIG, 0, 0
    for r, c in enumerate(int(v) for v in cand):
        det = {}
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d, sh = ref.distance(pp, q_desc, desc[c], q_pos if prior else np.zeros(2), pos[c] if prior else np.ones(2),
                                 q_dist if prior else 0.0, dist[c] if prior else 1.0, det)
        out["ties"] = out["ties"] or det["vkey_tie"] or det["shift_tie"]
        out["cand_id"][r], out["cand_yaw"][r], out["cand_dist"][r] = c, yaw_of(sh, S), d
        if d < min_d:
            min_d, nn_align, nn_idx = d, sh, c
    out.update(loop=nn_idx if min_d < p["dist_thresh"] else -1, yaw=yaw_of(nn_align, S), min_dist=min_d)
    return out


def split(cs, queries, drop=()):
    """a set of scancontext_cases as (database, queries): the nodes `queries` leave the database and query it, the nodes
    `drop` leave it too.  A query keeps its own odometry, so no candidate shares its traversed distance."""
    n = len(cs["desc"])
    keep = np.array([i for i in range(n) if i not in set(queries) | set(drop)])
    q = np.array(sorted(queries))
    db = dict(desc=cs["desc"][keep], rk=cs["rk"][keep], pos=cs["pos"][keep], dist=cs["dist"][keep])
    qs = dict(desc=cs["desc"][q], rk=cs["rk"][q], pos=cs["pos"][q], dist=cs["dist"][q])
    return db, qs


# the shapes of the parity tests: a descriptor that is staged in LDS and one that is not (asserted from branches())
PARITY_SETS = ("staged_max", "unstaged_min", "indoor_600")
N_PARITY_QUERIES = 5


@functools.lru_cache(maxsize=None)
def parity_case(name, decided):
    """(p, database, queries) of a parity test.  decided: the planted nodes (all-zero, periodic and never-meeting
    descriptors: ties between shifts BY CONSTRUCTION of the descriptor, which the reference reports as ties) leave the
    database, and the queries are the first unplanted nodes from the middle of the set."""
    cs = cases.make_set(name)
    n = len(cs["desc"])
    planted = set(cs["planted"].values())
    free = [i for i in range(n // 3, n) if i not in planted]
    queries = free[:: max(1, len(free) // N_PARITY_QUERIES)][:N_PARITY_QUERIES]
    if not decided:
        queries = queries[:-1] + [cs["planted"]["periodic_query"]]          # composition: a planted tie goes through both entries
    db, qs = split(cs, queries, planted if decided else ())
    return cs["p"], db, qs


@functools.lru_cache(maxsize=None)
def chunk_case():
    """4 x 8 descriptors, 3 chunks + 17 entries, num_candidates 5.  Every entry is a sector roll of one of a few integer
    places, so its ring key IS the place's key and equal distances are everywhere; on top, copies of four query places are
    planted at chosen slots.  Returns (p, database, queries, planted {query name: the indices of its copies})."""
    C = chunk_length()
    n, R, S, K = 3 * C + 17, 4, 8, 5
    rng = np.random.default_rng(4242)
    cfg = dict(R=R, S=S, search_ratio=1.2, num_candidates=K, num_exclude_recent=1, odom_weight=0.0)
    p = cases.params(cfg)
    places = [rng.integers(20, 60, (S, R)).astype(np.float64) for _ in range(40)]     # the crowd: keys far from the queries'
    desc = np.stack([np.roll(places[rng.integers(40)], int(rng.integers(S)), axis=0) for _ in range(n)])
    qplaces = {k: rng.integers(1, 9, (S, R)).astype(np.float64) + 100.0 * (j + 1) for j, k in enumerate(("tail", "per_chunk", "boundary", "inside"))}
    planted = {
        "tail": [3 * C + 2, 3 * C + 3, 3 * C + 9, 3 * C + 10, 3 * C + 15, 3 * C + 16],        # more copies than ranks, all in the ragged tail (its last slot too)
        "per_chunk": [7, C + 7, 2 * C + 7, 3 * C + 7],                                      # one per chunk; the fifth rank comes from the crowd
        "boundary": [C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1, 3 * C],                         # both sides of all three boundaries: the cut falls between equal distances
        "inside": [C + 100, C + 101, C + 102, C + 103, C + 104, C + 105, 0],               # neighbours inside chunk 1, and slot 0
    }
    for k, idx in planted.items():
        for i in idx:
            desc[i] = np.roll(qplaces[k], int(rng.integers(S)), axis=0)
    rk = cases.keys_of(desc)
    pos = np.cumsum(rng.normal(0, 0.4, (n, 2)), axis=0)
    dist = np.cumsum(rng.uniform(0.3, 0.7, n))
    order = list(planted)
    q_desc = np.stack([qplaces[k] for k in order] + [places[0]])                             # the last query: a crowd place, ties all over
    qs = dict(desc=q_desc, rk=cases.keys_of(q_desc), pos=rng.normal(0, 3, (len(q_desc), 2)), dist=dist[-1] + 5.0 + np.arange(len(q_desc)))
    for a in (desc, rk, pos, dist, *qs.values()):
        a.setflags(write=False)
    return p, dict(desc=desc, rk=rk, pos=pos, dist=dist), qs, {k: sorted(v) for k, v in planted.items()}


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """scancontext_cases.make_nonfinite_set tiled over more than a chunk: the nodes with a NaN key at slot 0, at the last slot
    of chunk 0, at the first slot of chunk 1 and at the last slot of the database; the node with an infinite key next to
    them.  Queries: finite nodes (node 17 is the one the infinite node copies), and a NaN node."""
    cs = cases.make_nonfinite_set()
    C = chunk_length()
    nan_a, nan_b = cs["planted"]["nan"]
    inf = cs["planted"]["inf"]
    finite = [i for i in range(len(cs["desc"])) if i not in (nan_a, nan_b, inf)]
    queries = [17, 20, 44]
    pool = [i for i in finite if i not in queries]
    n = C + 40
    src = np.array([pool[i % len(pool)] for i in range(n)])
    src[[0, C - 1, C, n - 1]] = [nan_a, nan_b, nan_a, nan_b]
    src[[1, C - 2, C + 1]] = inf
    rng = np.random.default_rng(9)
    db = dict(desc=cs["desc"][src], rk=cs["rk"][src], pos=np.cumsum(rng.normal(0, 0.4, (n, 2)), axis=0), dist=np.cumsum(rng.uniform(0.3, 0.7, n)))
    q = np.array(queries + [nan_a])
    qs = dict(desc=cs["desc"][q], rk=cs["rk"][q], pos=rng.normal(0, 3, (len(q), 2)), dist=db["dist"][-1] + 1.0 + np.arange(len(q)))
    return cs["p"], db, qs, dict(nan=[0, C - 1, C, n - 1], inf=[1, C - 2, C + 1], nan_query=len(q) - 1)


@functools.lru_cache(maxsize=None)
def nonfinite_small_case():
    """fewer valid entries than ranks: two finite nodes, the node with the infinite key between them, a NaN node first and
    last.  The infinite key distance is a distance: its node ranks behind the finite ones; the NaN nodes have no rank."""
    p, db, qs, info = nonfinite_case()
    fin = [i for i in range(2, 12) if i not in info["nan"] + info["inf"]][:2]
    idx = np.array([info["nan"][0], fin[0], info["inf"][0], fin[1], info["nan"][1]])
    return p, {k: v[idx] for k, v in db.items()}, qs, dict(nan=[0, 4], inf=2, finite=[1, 3])
