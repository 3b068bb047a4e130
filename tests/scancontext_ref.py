"""SCManager (Scancontext.cpp of the reference) restated a second time, in numpy float64 -- test infrastructure only.  No
oracle, no HIP library: the oracle (oracle/randt_oracle.c) is held to this file on the CPU before a kernel is judged by the
oracle.  Written differently from the oracle on purpose:

circshift (:39-59)              np.roll along the sector axis (a table of rolled column indices, one gather per candidate)
distDirectSC (:69-90)           every shift of the search space at once: column dots and norms as array operations, the
                                skipped all-zero sectors as terms of exactly 0.0 in the running sum
fastAlignUsingVkey (:93-113)    the S x S matrix of squared key differences, np.argmin (= the first minimum)
distanceBtnScanContext          the search space as the reference builds it: a sorted list, duplicates kept (:123-130)
detectLoopClosureID (:256-341)  float32 key distances accumulated ring by ring, the candidates by a stable
                                np.lexsort((index, distance)); "cur < min" on 10000000 as the reference writes it

Every sum the reference runs as a loop is an np.add.accumulate here (sequential, left to right), so the restatement carries
the reference's exact ties between shifts and between candidates instead of splitting them in the last bit.

Descriptors are stored desc[sector][ring] (a sector = the reference's matrix column).

NaN RULE (decision 13): a database entry whose float key distance to the query is not >= 0 (NaN) is never a
candidate; when no candidate is left the remaining ranks are absent.  A +inf distance is a distance: it sorts last."""
import functools

import numpy as np

BIG = 10000000.0


def _seq_sum(a, axis):
    """left-to-right sum along `axis` (np.sum adds pairwise)"""
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


@functools.lru_cache(maxsize=None)
def _rolled_columns(S):
    """row s = the column indices of a descriptor circularly shifted right by s sectors"""
    return np.stack([np.roll(np.arange(S), s) for s in range(S)])


def ring_key(desc):
    return _seq_sum(desc, 0) / desc.shape[0]


def sector_key(desc):
    return _seq_sum(desc, 1) / desc.shape[1]


def search_radius(search_ratio, S):
    return int(np.floor(0.5 * search_ratio * S + 0.5))          # round(): half away from zero, the argument is >= 0


def align_sector_keys(k1, k2):
    """fastAlignUsingVkey: (argmin shift, the S diff norms)"""
    S = len(k1)
    with np.errstate(invalid="ignore"):                                          # (inf - inf of an infinite key: NaN, never < )
        diff = k1[None, :] - k2[_rolled_columns(S)]
        norms = np.sqrt(_seq_sum(diff * diff, 1))
    ok = norms < BIG
    return (int(np.argmin(np.where(ok, norms, np.inf))) if ok.any() else 0), norms


def search_space(argmin_vkey, radius, S):
    space = [argmin_vkey]
    for ii in range(1, radius + 1):
        space.append((argmin_vkey + ii + S) % S)
        space.append((argmin_vkey - ii + S) % S)
    return sorted(space)


def shift_distances(sc1, sc2, shifts):
    """distDirectSC(sc1, circshift(sc2, s)) for every s in `shifts`"""
    S = sc1.shape[0]
    rolled = _rolled_columns(S)[np.asarray(shifts, dtype=np.int64)]              # [n_shift][S]: column c of sc2 shifted by s
    n1 = np.sqrt(_seq_sum(sc1 * sc1, 1))[None, :]
    n2 = np.sqrt(_seq_sum(sc2 * sc2, 1))[rolled]
    dot = np.zeros(rolled.shape)
    counted = (n1 != 0) & (n2 != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(sc1.shape[1]):                                            # ring by ring: the reference's order
            dot = dot + sc1[None, :, r] * sc2[:, r][rolled]
        sim = np.where(counted, dot / (n1 * n2), 0.0)
        return 1.0 - _seq_sum(sim, 1) / counted.sum(axis=1)                       # 0 / 0 = NaN when no sector counts


def distance(p, sc1, sc2, pos1, pos2, dist1, dist2, detail=None):
    """distanceBtnScanContext: (distance, argmin shift).  p: a dict with the randt_sc_params fields."""
    S, R = sc1.shape
    argmin_vkey, norms = align_sector_keys(sector_key(sc1), sector_key(sc2))
    space = search_space(argmin_vkey, search_radius(p["search_ratio"], S), S)
    d = shift_distances(sc1, sc2, space)
    argmin_shift, min_sc = 0, BIG
    for s, v in zip(space, d):
        if v < min_sc:
            argmin_shift, min_sc = s, float(v)
    dx, dy = float(pos2[0] - pos1[0]), float(pos2[1] - pos1[1])
    t_err = max(float(np.sqrt(dx * dx + dy * dy)) - p["odom_eps"], 0.0) / float(dist2 - dist1)
    odom = 1.0 - np.exp(-(t_err * t_err) / (2 * p["assumed_drift"] * p["assumed_drift"]))
    if detail is not None:
        ok = norms[norms < BIG]
        detail["vkey_tie"] = bool(len(ok) and (ok == ok.min()).sum() > 1)
        dd = d[np.unique(space, return_index=True)[1]]                            # one entry per distinct shift
        dd = dd[dd < BIG]
        detail["shift_tie"] = bool(len(dd) and (dd == dd.min()).sum() > 1)
        detail["shift"] = argmin_shift
    return min_sc + odom * R * p["odom_weight"], argmin_shift


def key_distances(ring_keys, node_id, n_search):
    """nanoflann's L2 adaptor on the float keys: squared differences accumulated in float32, ring by ring"""
    rk = np.asarray(ring_keys, dtype=np.float64).astype(np.float32)
    acc = np.zeros(n_search, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rk.shape[1]):
            d = rk[node_id, r] - rk[:n_search, r]
            acc = acc + d * d
    assert acc.dtype == np.float32
    return acc


def candidates(p, ring_keys, node_id):
    """the k nearest keys of the searchable database in (distance, index) order, and all the distances"""
    n_search = node_id + 1 - p["num_exclude_recent"]
    d2 = key_distances(ring_keys, node_id, n_search)
    idx = np.arange(n_search)
    order = np.lexsort((idx, d2))
    with np.errstate(invalid="ignore"):
        order = order[d2[order] >= 0]                                             # the NaN rule (+inf stays)
    return order[: p["num_candidates"]], d2


def detect(p, desc, ring_keys, pos, dist, node_id, detail=None):
    """detectLoopClosureID: (loop id or -1, yaw difference as float32, minimal distance)"""
    n_db, S, R = desc.shape
    if node_id < p["num_exclude_recent"] + 1 or node_id >= n_db:
        return -1, np.float32(0.0), BIG
    cand, d2 = candidates(p, ring_keys, node_id)
    min_d, nn_align, nn_idx = BIG, 0, 0
    totals, sub = [], []
    for c in cand:
        dd = {} if detail is not None else None
        d, sh = distance(p, desc[node_id], desc[c], pos[node_id], pos[c], dist[node_id], dist[c], dd)
        totals.append(d)
        sub.append(dd)
        if d < min_d:
            min_d, nn_align, nn_idx = d, sh, int(c)
    if detail is not None:
        detail.update(candidates=np.array(cand), totals=np.array(totals), per_candidate=sub, d2=d2)
    yaw = np.float32(float(np.float32(nn_align * (360.0 / S))) * np.pi / 180.0)   # deg2rad of a float angle, in double (:17-20, :336)
    return (nn_idx if min_d < p["dist_thresh"] else -1), yaw, min_d
