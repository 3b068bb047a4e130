"""The pair solve (solve.hip k_solve / k_solve_order, solve_pass.h eval_pass) above one scan's worth of cells.  Every other
parity test registers maps of 45-76 cells against fixed batches of capacity <= 10000: at most ~300 residuals, always the
compacted list with packed 16-bit record offsets, never the sorted placement.  Here:

A. record addressing -- packed 16-bit offsets (3 cap <= 65536), (moving << 21) | fixed, and the raw-slot walk (n_res > 1024,
   M > 2048 or cap > 2^21), at each boundary between them; every instantiation on the two rarely taken forms; table entries
   outside [0, cap) in each of the three.
B. sorted placement -- k_solve_order and the order[slot] indirection (RANDT_SOLVE_GROUP=1, ragged batches, more than one
   stride of the order kernel) against the unsorted one-registration-per-workgroup launch, bit for bit.

Reference: the CPU oracle's solve on the SAME correspondence table (po.solve_pair), at the bars of test_gpu_parity.py: pose
1e-7 absolute, cost and trace 1e-8 relative, equal residual / iteration / termination counts.  Where two launches walk the
same list with the same lane assignment they must agree bit for bit.  The unmarked tests pin the inputs on the oracle alone
(size classes, masks, conditioning), so they run without a GPU."""
import functools
import os

import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import synth
from util import IP, oracle_scan_map, oracle_submap, problem, to_oracle_params

PAIR_CAP = 1024                    # solve_pass.h: compacted correspondences per registration
PAIR_SHIFT = 21                    # ... and the moving index's position in the wide form
MCAP = 4096                        # moving-batch capacity: M k > 2048 keeps the split-mode kernel out of every launch here
TRACE_LEN = 3 * 512 + 1
TRUE3 = np.array([0.12, -0.08, 0.02])                 # (x, y, theta) of the moving frame in the fixed one; also the guess
G4 = synth.pose3_to_pose4(TRUE3)
#          name (the measured cell count), half width of the cut-out, neighbours per cell
MOVING = (("m53", 4.0, 4), ("m285", 8.5, 4), ("m549", 12.0, 4), ("m2241", 23.9, 4), ("m84", 5.0, 12), ("m2048", None, 4))
I53, I285, I549, I2241, I84, I2048 = range(6)       # m2048: the first 2048 cells of m2241 -- the largest map that is still compacted
CAPS = (10000, 21845, 21846, (1 << PAIR_SHIFT) + 1)   # 21845 = the last capacity with 16-bit offsets, 2^21 + 1 = the first raw walk
INT_MIN = -2 ** 31


def dense_omap(cap):
    return po.Map(IP["size_x"], IP["size_y"], IP["resolution"], (0.0, 0.0), IP["max_neighbour_dist"], 3, cap)


@functools.lru_cache(maxsize=None)
def dense():
    """40000 uniform points -> one cell per 1 m cluster of the 48 m square (2209 cells); moving maps: the same points inside
    |x|, |y| < half, jittered by 1 cm, seen from TRUE3."""
    rng = np.random.default_rng(7)
    pts = np.zeros((40000, 4), dtype=np.float32)
    pts[:, :2] = rng.uniform(-23.9, 23.9, (40000, 2))
    pts[:, 3] = rng.uniform(10.0, 90.0, 40000)
    fixed = dense_omap(10000)
    fixed.build(pts, 2304, 24.0)
    inv = synth.se2_inv3(TRUE3)
    c, s = np.cos(inv[2]), np.sin(inv[2])
    moving = []
    for _, half, _ in MOVING:
        if half is None:
            m = dense_omap(MCAP)
            m.set(moving[I2241].cells()[:2048], np.full(m.n_slots, -1, dtype=np.int32))
            moving.append(m)
            continue
        q = pts[(np.abs(pts[:, 0]) < half) & (np.abs(pts[:, 1]) < half)].copy()
        q[:, :2] += np.random.default_rng(8).normal(0, 0.01, (len(q), 2)).astype(np.float32)
        x, y = c * q[:, 0] - s * q[:, 1] + inv[0], s * q[:, 0] + c * q[:, 1] + inv[1]
        q[:, 0], q[:, 1] = x, y
        m = dense_omap(MCAP)
        m.build(q, 2304, 24.0)
        moving.append(m)
    return fixed, moving


@functools.lru_cache(maxsize=None)
def oracle_table(i):
    fixed, moving = dense()
    corr, n = po.associate(fixed, moving[i], G4, MOVING[i][2], 1, 1)
    assert n == (corr >= 0).sum()
    return corr


def masked(table, n_keep, seed):
    """`table` with a seeded choice of n_keep valid entries left, the others -1: the moving map (M) stays what it was"""
    valid = np.flatnonzero(table.reshape(-1) >= 0)
    keep = np.random.default_rng(seed).choice(valid, n_keep, replace=False)
    out = np.full(table.shape, -1, dtype=np.int32)
    out.reshape(-1)[keep] = table.reshape(-1)[keep]
    return out


BOUNDARY = (1023, 1024, 1025, 1140)


def boundary_table(n_res):
    t = oracle_table(I285)
    return t if n_res == (t >= 0).sum() else masked(t, n_res, 100 + n_res)


def sparse_2241_table():
    return masked(oracle_table(I2241), 1000, 2241)


def sparse_2048_table():
    return masked(oracle_table(I2048), 1000, 2048)


def raised(table, cap, n_fixed):
    """the table for a fixed map whose n_fixed cells sit at the TOP of a batch of capacity cap"""
    return np.where(table >= 0, table + (cap - n_fixed), -1).astype(np.int32)


TOP_CAPS = (21845, 21846, 1 << PAIR_SHIFT)      # the largest record offsets of the 16-bit form, and of the 21-bit form


def garbage_tables(table, cap, seed):
    """(dirty, clean): sixteen valid entries (the dense tables have no others) replaced by values outside [0, cap) -- cap,
    cap + 5, -7, INT_MIN in turn -- and the same entries set to -1."""
    pos = np.random.default_rng(seed).choice(np.flatnonzero(table.reshape(-1) >= 0), 16, replace=False)
    dirty, clean = table.copy(), table.copy()
    dirty.reshape(-1)[pos] = np.resize(np.array([cap, cap + 5, -7, INT_MIN], dtype=np.int64), len(pos)).astype(np.int32)
    clean.reshape(-1)[pos] = -1
    return dirty, clean


#                path          moving map, fixed capacity, table
GARBAGE = {"pack16": (I53, 10000), "wide21": (I53, 21846), "raw": (I285, 10000)}


def garbage_case(path):
    i, cap = GARBAGE[path]
    return (i, cap) + garbage_tables(oracle_table(i), cap, 300 + i + cap)


def addressing(M, n_res, cap):
    """the form k_solve's prologue chooses (solve.hip), from the sizes alone"""
    if n_res == 0:
        return "none"
    if n_res > PAIR_CAP or cap > (1 << PAIR_SHIFT) or M > (1 << (32 - PAIR_SHIFT)):
        return "raw"
    return "pack16" if 3 * cap <= 65536 and 3 * M <= 65536 else "wide21"


def oracle_solve(i, table, mp, guess=G4):
    fixed, moving = dense()
    return po.solve_pair(fixed, moving[i], table, to_oracle_params(mp), guess)


# ------------------------------------------------------------------ CPU: the inputs, on the oracle alone ----------
def test_dense_pair_size_classes(built):
    fixed, moving = dense()
    M = [m.n_cells for m in moving]
    n_res = [int((oracle_table(i) >= 0).sum()) for i in range(len(MOVING))]
    print("fixed cells", fixed.n_cells, "M", M, "n_res", n_res)
    assert [n for n, _, _ in MOVING] == ["m%d" % m for m in M]
    assert fixed.n_cells == 2209 and all(oracle_table(i).max() < fixed.n_cells for i in range(len(MOVING)))
    assert M[I53] < 256 and n_res[I53] <= PAIR_CAP and n_res[I84] <= PAIR_CAP and n_res[I84] > 900 and MOVING[I84][2] == 12
    assert 256 < M[I285] <= 2048 and n_res[I285] > PAIR_CAP                    # the raw walk through n_res alone
    assert 256 < M[I549] <= 2048 and n_res[I549] > 2 * PAIR_CAP
    assert M[I2241] > 2048 and M[I2241] <= MCAP and n_res[I2241] > PAIR_CAP     # ... and through M
    assert M[I2048] == 2048 == 1 << (32 - PAIR_SHIFT) and np.array_equal(oracle_table(I2048), oracle_table(I2241)[:2048])
    assert [addressing(M[i], n_res[i], 10000) for i in range(6)] == ["pack16", "raw", "raw", "raw", "pack16", "raw"]
    assert [addressing(M[I53], n_res[I53], c) for c in CAPS] == ["pack16", "pack16", "wide21", "raw"]
    assert [addressing(M[I84], n_res[I84], c) for c in CAPS] == ["pack16", "pack16", "wide21", "raw"]
    assert 3 * CAPS[1] <= 65536 < 3 * CAPS[2] and CAPS[3] - 1 == 1 << PAIR_SHIFT


def test_masked_tables_sit_on_both_sides_of_the_boundaries(built):
    _, moving = dense()
    for n in BOUNDARY:
        t = boundary_table(n)
        assert t.shape == (moving[I285].n_cells, 4) and (t >= 0).sum() == n
        assert addressing(len(t), n, 10000) == ("pack16" if n <= PAIR_CAP else "raw")
        assert addressing(len(t), n, 21846) == ("wide21" if n <= PAIR_CAP else "raw")
    t = sparse_2241_table()
    rows = np.flatnonzero((t >= 0).any(axis=1))
    print("M = 2241 masked: n_res", (t >= 0).sum(), "rows >= 2048 with an entry:", (rows >= 2048).sum())
    assert (t >= 0).sum() == 1000 <= PAIR_CAP and (rows >= 2048).sum() >= 20     # only M > 2048 forbids the compaction
    assert addressing(len(t), 1000, 10000) == "raw"
    t = sparse_2048_table()
    rows = np.flatnonzero((t >= 0).any(axis=1))
    print("M = 2048 masked: n_res", (t >= 0).sum(), "rows >= 1024 with an entry:", (rows >= 1024).sum(), "last row", rows.max())
    assert (t >= 0).sum() == 1000 and (rows >= 1024).sum() >= 100 and rows.max() >= 2040    # the top bit of the 11-bit moving index is in use
    assert addressing(len(t), 1000, 10000) == "pack16" and addressing(len(t), 1000, 21846) == "wide21"
    n_fixed = dense()[0].n_cells
    for cap in TOP_CAPS:                                                     # record indices that need every bit of their field
        for i in (I53, I84):
            r = raised(oracle_table(i), cap, n_fixed)
            v = r[r >= 0]
            assert len(v) == (oracle_table(i) >= 0).sum() and v.max() < cap and v.max() >= cap - 1200
            if cap == 21845:
                assert addressing(len(r), len(v), cap) == "pack16" and 3 * v.max() > 65536 - 3 * 1200 and (3 * v >= 1 << 15).all()
            else:
                assert addressing(len(r), len(v), cap) == "wide21" and (cap < 1 << 20 or (v >= 1 << 20).all())
    for path in GARBAGE:
        i, cap, dirty, clean = garbage_case(path)
        bad = dirty[dirty != clean]
        assert len(bad) == 16 and set(bad.tolist()) == {cap, cap + 5, -7, INT_MIN} and (clean[dirty != clean] == -1).all()
        assert addressing(len(clean), int((clean >= 0).sum()), cap) == path
        assert ((dirty >= 0) & (dirty < cap)).sum() == (clean >= 0).sum() == (oracle_table(i) >= 0).sum() - 16


def test_oracle_solves_are_well_conditioned(built):
    """status 0 everywhere; a 1e-12 change of the guess moves the result by far less than the 1e-7 the device is held to
    (measured: <= 7e-11), so that bar does not depend on which of two nearby roundings a pass takes."""
    cases = [(i, oracle_table(i)) for i in range(len(MOVING))] + [(I285, boundary_table(n)) for n in BOUNDARY[:3]]
    cases += [(I2241, sparse_2241_table()), (I2048, sparse_2048_table())]
    cases += [(garbage_case(p)[0], garbage_case(p)[3]) for p in GARBAGE]
    for i, t in cases:
        mp = R.default_matcher_params(n_neighbours=MOVING[i][2])
        rc, p4, st = oracle_solve(i, t, mp)
        rc2, q4, _ = oracle_solve(i, t, mp, G4 + np.array([0.0, 0.0, 1e-12, -1e-12]))
        print(MOVING[i][0], "n_res", st["n_residuals"], "iterations", st["n_iterations"], "moved", np.abs(p4 - q4).max())
        assert rc == 0 and rc2 == 0 and st["n_residuals"] == (t >= 0).sum() and st["termination"] in (1, 2, 3)
        assert np.abs(p4 - q4).max() <= 1e-9
        assert np.abs(synth.pose4_to_pose3(p4) - TRUE3).max() < 0.1           # and it is a registration: within a tenth of a 1 m cluster of the true transform


# ---- B: the mixed batch
N_RAGGED, N_MANY = 75, 1100          # 75: no multiple of 2, 4 or 8; 1100: beyond one stride of the 1024-thread order kernel


@functools.lru_cache(maxsize=None)
def mixed_layout():
    """type of every moving map of the batch: 0..7 the rig's scans of submap 0, 8 empty, 9 the M = 285 map, 10 the M = 2241 map.
    Maps [0, 75): everything; [75, 75 + 1100): scans and empty maps only."""
    head = np.array([10] * 3 + [9] * 6 + [8] * 10 + [i % 8 for i in range(N_RAGGED - 19)])
    head = head[np.random.default_rng(21).permutation(N_RAGGED)]
    tail = np.random.default_rng(22).integers(0, 9, N_MANY)
    return np.concatenate([head, tail])


@functools.lru_cache(maxsize=None)
def mixed_types():
    """per type: (oracle moving map, fixed map of the pair, guess)"""
    prob = problem()
    assert (prob["submap_of"][:8] == 0).all()
    _, moving = dense()
    types = [(oracle_scan_map(prob["scans"][i]), 1, synth.pose3_to_pose4(prob["guess"][i])) for i in range(8)]
    return types + [(dense_omap(8), 1, G4), (moving[I285], 0, G4), (moving[I2241], 0, G4)]


def trips(M, k=4):
    return (M * k + 63) >> 6


def test_mixed_batch_layout(built):
    lay, types = mixed_layout(), mixed_types()
    assert len(lay) == N_RAGGED + N_MANY and all(N_RAGGED % r for r in (2, 4, 8)) and N_MANY > 1024 and N_MANY % 4 == 0
    assert set(lay[:N_RAGGED]) == set(range(11)) and set(lay[N_RAGGED:]) == set(range(9))
    M = [t[0].n_cells for t in types]
    print("cells per type", M, "trips", [trips(m) for m in M])
    assert M[8] == 0 and all(0 < m < 128 for m in M[:8])                  # one scan's worth
    keys = [63 - min(trips(m), 63) for m in M]                                  # k_solve_order's histogram key
    assert trips(M[10]) > 63 and keys[10] == 0 and keys[8] == 63 and len(set(keys)) >= 4
    # the sort has something to do: the batch is not already in descending order of size
    k75 = [keys[t] for t in lay[:N_RAGGED]]
    assert k75 != sorted(k75)


# ------------------------------------------------------------------ GPU ----------
def ctx_with(torch, env=None, mode=None):
    """A context created under the given environment knobs (they are read at creation) / solve mode."""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if mode is not None:
        ctx.set_solve_mode(mode)
    return ctx


def view(ctx, maps):
    """the same device storage as a batch of another context"""
    if maps.ctx is ctx:
        return maps
    return R.Maps(ctx, maps.n_maps, maps.params, maps.capacity, storage=maps.device_ptrs(), clear=False)


class Rig:
    def __init__(self):
        import torch

        self.torch, self.dev = torch, torch.device("cuda:0")
        self.ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
        self.mapp = R.MapParams(IP["size_x"], IP["size_y"], IP["resolution"], 0.0, 0.0, IP["max_neighbour_dist"], 3, 0)
        self.ofixed, self.omoving = dense()
        self.mm = R.Maps(self.ctx, len(MOVING), self.mapp, MCAP, with_grid=False)
        for i, m in enumerate(self.omoving):
            self.mm.upload(i, m.cells())
        self._fixed, self._ctx = {}, {}
        self.tables = self.associate(4, 0, 4) + self.associate(12, 4, 1) + self.associate(4, 5, 1)    # the device's own association

    def fixed(self, cap, n_maps=2):
        """the dense fixed map as map 0 of a batch of capacity `cap` (a second, empty map behind it: a record index of
        cap + 5, should one ever be followed, stays inside the allocation)"""
        if cap not in self._fixed:
            fm = R.Maps(self.ctx, n_maps, self.mapp, cap, with_grid=True)
            fm.upload(0, self.ofixed.cells(), self.ofixed.grid())
            self._fixed[cap] = fm
        return self._fixed[cap]

    def context(self, **env):
        key = tuple(sorted(env.items()))
        if key not in self._ctx:
            self._ctx[key] = ctx_with(self.torch, env) if env else self.ctx
        return self._ctx[key]

    def associate(self, k, first, n):
        torch = self.torch
        mp = R.default_matcher_params(n_neighbours=k)
        guess = torch.from_numpy(np.tile(G4, (n, 1))).to(self.dev)
        corr = torch.full((n, MCAP, k), -7, dtype=torch.int32, device=self.dev)
        R.associate_batch(self.ctx, self.fixed(10000), torch.zeros(n, dtype=torch.int32, device=self.dev), self.mm, first, n, guess, mp, corr)
        self.ctx.synchronize()
        corr = corr.cpu().numpy()
        return [corr[j, :self.omoving[first + j].n_cells].copy() for j in range(n)]

    def solve(self, fm, first, tables, mp, ctx=None):
        """solve_batch of moving maps [first, first + len(tables)) against map 0 of fm with explicit tables, from G4"""
        torch = self.torch
        ctx = ctx or self.ctx
        n, k = len(tables), mp.n_neighbours
        corr = np.full((n, MCAP, k), -1, dtype=np.int32)
        for j, t in enumerate(tables):
            assert t.shape == (self.omoving[first + j].n_cells, k)
            corr[j, :len(t)] = t
        pose = torch.from_numpy(np.tile(G4, (n, 1))).to(self.dev)
        res = torch.full((n, 64), 0xA5, dtype=torch.uint8, device=self.dev)
        trace = torch.zeros((n, TRACE_LEN), dtype=torch.float64, device=self.dev)
        ctx.set_trace(trace, TRACE_LEN)
        R.solve_batch(ctx, view(ctx, fm), torch.zeros(n, dtype=torch.int32, device=self.dev), view(ctx, self.mm), first, n,
                      torch.from_numpy(corr).to(self.dev), mp, pose, res)
        ctx.synchronize()
        ctx.set_trace(None, 0)
        return pose.cpu().numpy(), res.cpu().numpy(), trace.cpu().numpy()


@pytest.fixture(scope="module")
def rig(built):
    return Rig()


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_oracle(out, j, i, table, mp, tag):
    """registration j of a launch against the oracle's solve of moving map i on `table` (which holds -1 or fixed indices)"""
    pose, res, trace = out
    r = res.view(R.RESULT_DTYPE).reshape(-1)[j]
    rc, p4, st = oracle_solve(i, table, mp)
    n = int(trace[j, 0])
    t = trace[j, 1:1 + 3 * n].reshape(n, 3)
    m = min(n, len(st["trace_cost"]))
    print("%s: n_res %d / %d, iterations %d / %d, termination %d / %d, pose diff %.3g, cost rel %.3g, trace rel %.3g" % (
        tag, r["n_residuals"], st["n_residuals"], r["iterations"], st["n_iterations"], r["termination"], st["termination"],
        np.abs(pose[j] - p4).max(), abs(r["final_cost"] / st["final_cost"] - 1.0), np.abs(t[:m, 0] / st["trace_cost"][:m] - 1.0).max()))
    assert rc == 0 and r["status"] == 0, tag
    assert np.allclose(pose[j], p4, rtol=0, atol=1e-7), (tag, pose[j], p4)
    assert r["n_residuals"] == st["n_residuals"] == (table >= 0).sum(), tag
    assert r["gnc_solves"] == st["n_solves"] and r["iterations"] == st["n_iterations"] and r["termination"] == st["termination"], tag
    assert np.isclose(r["final_cost"], st["final_cost"], rtol=1e-8) and np.isclose(r["cost"], st["final_cost"] / st["n_residuals"], rtol=1e-8), tag
    assert n == len(st["trace_cost"]) and 3 * n + 1 <= TRACE_LEN, tag
    assert np.allclose(t[:, 0], st["trace_cost"], rtol=1e-8) and np.allclose(t[:, 1], st["trace_radius"], rtol=1e-8), tag
    assert np.array_equal(t[:, 2].astype(int), st["trace_flag"]), tag


@pytest.mark.gpu
def test_association_of_the_dense_maps_equals_the_oracle(rig):
    """associate_batch at M = 53 .. 2241 (up to 36 chunks per workgroup) and k = 12 (the WIDE instantiation): the tables
    every test below starts from"""
    for i in range(len(MOVING)):
        assert np.array_equal(rig.tables[i], oracle_table(i)), MOVING[i][0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_res", BOUNDARY)
def test_pair_cap_boundary(rig, n_res):
    """M = 285 on both sides of PAIR_CAP: 1023 and 1024 residuals are compacted (16-bit offsets at capacity 10000, the 21-bit
    form at 21846 -- the same list, so the same bits), 1025 and 1140 walk the raw slots at either capacity."""
    mp = R.default_matcher_params()
    t = rig.tables[I285] if n_res == 1140 else boundary_table(n_res)
    a = rig.solve(rig.fixed(10000), I285, [t], mp)
    b = rig.solve(rig.fixed(21846), I285, [t], mp)
    check_oracle(a, 0, I285, t, mp, "cap 10000, n_res %d" % n_res)
    check_oracle(b, 0, I285, t, mp, "cap 21846, n_res %d" % n_res)
    assert same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["full", "masked"])
def test_more_than_2048_moving_cells(rig, which):
    """M = 2241: the moving index no longer fits the 11 bits above PAIR_SHIFT.  full: 8964 residuals, 141 trips per pass;
    masked: 1000 residuals, entries at moving indices >= 2048 -- few enough to compact, were it not for M."""
    mp = R.default_matcher_params()
    t = rig.tables[I2241] if which == "full" else sparse_2241_table()
    for cap in (10000, 21846):
        check_oracle(rig.solve(rig.fixed(cap), I2241, [t], mp), 0, I2241, t, mp, "M 2241 %s, cap %d" % (which, cap))


@pytest.mark.gpu
def test_2048_moving_cells_are_still_compacted(rig):
    """M = 2048, 1000 residuals up to moving index 2047: the last map whose index fits above PAIR_SHIFT, in either form"""
    mp = R.default_matcher_params()
    t = sparse_2048_table()
    a = rig.solve(rig.fixed(10000), I2048, [t], mp)
    b = rig.solve(rig.fixed(21846), I2048, [t], mp)
    check_oracle(a, 0, I2048, t, mp, "M 2048, cap 10000")
    check_oracle(b, 0, I2048, t, mp, "M 2048, cap 21846")
    assert same_bits(a, b)


@pytest.fixture(scope="module")
def capacity_runs(rig):
    """the 212- (k = 4) and the 1008-residual (k = 12) registration against the same fixed cells in batches of every capacity"""
    out = {}
    for cap in CAPS:
        big = cap > 100000
        fm = rig.fixed(cap, 1 if big else 2)                 # 2^21 + 1 cells: 100 MB
        for i in (I53, I84):
            mp = R.default_matcher_params(n_neighbours=MOVING[i][2])
            out[(cap, i)] = rig.solve(fm, i, [rig.tables[i]], mp)
        if big:
            rig._fixed.pop(cap).close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("i", [I53, I84], ids=["k4", "k12"])
def test_fixed_capacity_boundaries(rig, capacity_runs, i):
    """10000 and 21845: 16-bit offsets; 21846: the first 21-bit capacity; 2^21 + 1: the raw walk.  The first three walk the
    same compacted list: same bits.  All four match the oracle."""
    mp = R.default_matcher_params(n_neighbours=MOVING[i][2])
    for cap in CAPS:
        check_oracle(capacity_runs[(cap, i)], 0, i, rig.tables[i], mp, "%s, cap %d" % (MOVING[i][0], cap))
    for cap in CAPS[1:3]:
        assert same_bits(capacity_runs[(cap, i)], capacity_runs[(CAPS[0], i)]), cap


@pytest.mark.gpu
@pytest.mark.parametrize("cap", TOP_CAPS)
def test_fixed_records_at_the_top_of_the_capacity(rig, capacity_runs, cap):
    """the same fixed cells uploaded as the LAST 2209 of a map that fills its capacity (zeroed records below them), the tables
    raised to match: record offsets up to 3 x 21844 in the 16-bit form, fixed indices with bit 20 set in the 21-bit form at
    capacity 2^21 -- the same list and lanes as at capacity 10000, so the same bits"""
    fc = rig.ofixed.cells()
    cells = np.zeros(cap, dtype=R.CELL_DTYPE)
    cells[cap - len(fc):] = fc
    fm = R.Maps(rig.ctx, 1, rig.mapp, cap, with_grid=False)
    fm.upload(0, cells)
    for i in (I53, I84):
        mp = R.default_matcher_params(n_neighbours=MOVING[i][2])
        got = rig.solve(fm, i, [raised(rig.tables[i], cap, len(fc))], mp)
        assert got[1].view(R.RESULT_DTYPE).reshape(-1)[0]["status"] == 0
        assert same_bits(got, capacity_runs[(CAPS[0], i)]), (cap, MOVING[i][0])
    fm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("param", [R.PARAM_AMBIENT4, R.PARAM_MANIFOLD, R.PARAM_VECTOR, R.PARAM_ANALYTIC])
@pytest.mark.parametrize("alpha", [-2.0, -1.0])
@pytest.mark.parametrize("intensity", [1, 0])
def test_instantiations_on_the_wide_and_the_raw_form(rig, intensity, alpha, param):
    """one launch of two registrations at capacity 21846 -- 212 residuals in the 21-bit form, 1140 on the raw walk -- for every
    residual dimension, loss form and parameterisation; four registrations per workgroup (the default), one, and two
    wavefronts per registration (RANDT_SOLVE_BLOCK=128: another lane assignment, so the oracle's bars only)."""
    mp = R.default_matcher_params(parameterization=param, use_intensity=intensity, loss_alpha=alpha)
    tables = [rig.tables[I53], rig.tables[I285]]
    fm = rig.fixed(21846)
    outs = {}
    for name, env in (("rpb4", {"RANDT_SOLVE_RPB": "4"}), ("rpb1", {"RANDT_SOLVE_RPB": "1"}), ("block128", {"RANDT_SOLVE_BLOCK": "128"})):
        outs[name] = rig.solve(fm, I53, tables, mp, rig.context(**env))
        for j, i in enumerate((I53, I285)):
            check_oracle(outs[name], j, i, tables[j], mp, "%s %s" % (name, MOVING[i][0]))
    assert same_bits(outs["rpb4"], outs["rpb1"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(GARBAGE))
def test_table_entries_outside_the_fixed_capacity(rig, path):
    """cap, cap + 5, -7 and INT_MIN in the table are no correspondences: not counted, not followed -- the same bits as -1 in
    their place, in the compaction of either form and on the raw walk."""
    i, cap, dirty, clean = garbage_case(path)
    mp = R.default_matcher_params()
    a = rig.solve(rig.fixed(cap), i, [dirty], mp)
    b = rig.solve(rig.fixed(cap), i, [clean], mp)
    check_oracle(b, 0, i, clean, mp, "%s, clean" % path)
    assert a[1].view(R.RESULT_DTYPE).reshape(-1)[0]["n_residuals"] == ((dirty >= 0) & (dirty < cap)).sum()
    assert same_bits(a, b)


# ---- B: sorted placement
class Mixed:
    def __init__(self, rig):
        torch = self.torch = rig.torch
        self.rig, self.dev = rig, rig.dev
        lay, types = mixed_layout(), mixed_types()
        self.n = len(lay)
        self.ref_ctx = ctx_with(torch, {"RANDT_SOLVE_GROUP": "0", "RANDT_SOLVE_RPB": "1"}, R._capi.SOLVE_THROUGHPUT)
        ctx = self.ref_ctx
        self.fm = R.Maps(ctx, 2, rig.mapp, 10000, with_grid=True)
        self.fm.upload(0, rig.ofixed.cells(), rig.ofixed.grid())
        sub = oracle_submap(problem()["submaps"][0])
        self.osub = sub
        self.fm.upload(1, sub.cells(), sub.grid())
        self.mm = R.Maps(ctx, self.n, rig.mapp, MCAP, with_grid=False)
        cells = [t[0].cells() for t in types]
        for j, t in enumerate(lay):
            self.mm.upload(j, cells[t])
        self.fidx = torch.from_numpy(np.array([types[t][1] for t in lay], dtype=np.int32)).to(self.dev)
        self.guess = np.stack([types[t][2] for t in lay])
        self.mp = R.default_matcher_params()
        self.corr = torch.full((self.n, MCAP, 4), -1, dtype=torch.int32, device=self.dev)
        R.associate_batch(ctx, self.fm, self.fidx, self.mm, 0, self.n, torch.from_numpy(self.guess).to(self.dev), self.mp, self.corr)
        ctx.synchronize()
        self.ref = {}

    def run(self, ctx, first, n, fill):
        """solve of maps [first, first + n); result and pose buffers with a guard row on either side, pre-filled"""
        torch = self.torch
        pose = torch.full((n + 2, 4), 7.0e77, dtype=torch.float64, device=self.dev)
        pose[1:-1] = torch.from_numpy(self.guess[first:first + n]).to(self.dev)
        res = torch.full((n + 2, 64), fill, dtype=torch.uint8, device=self.dev)
        trace = torch.zeros((n, TRACE_LEN), dtype=torch.float64, device=self.dev)
        ctx.set_trace(trace, TRACE_LEN)
        R.solve_batch(ctx, view(ctx, self.fm), self.fidx[first:first + n], view(ctx, self.mm), first, n, self.corr[first:first + n], self.mp,
                      pose[1:-1], res[1:-1])
        ctx.synchronize()
        ctx.set_trace(None, 0)
        pose, res = pose.cpu().numpy(), res.cpu().numpy()
        assert (pose[[0, -1]] == 7.0e77).all() and (res[[0, -1]] == fill).all()          # nothing outside the batch is written
        return pose[1:-1], res[1:-1], trace.cpu().numpy()

    def reference(self, first, n):
        """RANDT_SOLVE_GROUP=0, one registration per workgroup; checked against the oracle once per type of map"""
        if (first, n) not in self.ref:
            out = self.run(self.ref_ctx, first, n, 0x11)
            pose, res, _ = out
            rec = res.view(R.RESULT_DTYPE).reshape(-1)
            lay, types = mixed_layout()[first:first + n], mixed_types()
            op = to_oracle_params(self.mp)
            for t, (om, f, g) in enumerate(types):
                at = np.flatnonzero(lay == t)
                if not len(at):
                    continue
                rc, p4, cost, st = po.register_pair(self.rig.ofixed if f == 0 else self.osub, om, op, g)
                j = at[0]
                assert rec["status"][j] == rc and rec["n_residuals"][j] == st["n_residuals"], t
                assert np.allclose(pose[j], p4, rtol=0, atol=1e-7) and rec["iterations"][j] == st["n_iterations"], t
                if rc == 0:
                    assert np.abs(pose[j] - g).max() > 1e-6, t                               # a solve moves the pose ...
                else:
                    assert np.array_equal(pose[j], g) and rec["n_residuals"][j] == 0, t      # ... an empty map leaves it
                for x in out:
                    assert (x[at] == x[j]).all(), t                                          # same inputs, same bits, wherever they sit
            self.ref[(first, n)] = out
        return self.ref[(first, n)]


@pytest.fixture(scope="module")
def mixed(rig):
    return Mixed(rig)


def check_sorted(mixed, first, n, rpb):
    ref = mixed.reference(first, n)
    ctx = ctx_with(mixed.torch, {"RANDT_SOLVE_GROUP": "1", "RANDT_SOLVE_RPB": str(rpb)}, R._capi.SOLVE_THROUGHPUT)
    got = mixed.run(ctx, first, n, 0xEE)           # another fill than the reference's 0x11: a byte nobody wrote differs
    rec = got[1].view(R.RESULT_DTYPE).reshape(-1)
    assert set(rec["status"].tolist()) <= {0, 1} and (rec["reserved"] == 0).all()
    for name, a, b in zip(("poses", "records", "traces"), got, ref):
        bad = np.flatnonzero((a != b).reshape(n, -1).any(axis=1))
        assert not len(bad), (name, rpb, bad[:10], mixed_layout()[first:first + n][bad[:10]])


@pytest.mark.gpu
@pytest.mark.parametrize("rpb", [2, 4, 8])
def test_sorted_placement_ragged_batch(mixed, rpb):
    """75 registrations of 0 .. 141 residual trips through k_solve_order: every one solved once, by the wavefront the order
    names -- poses, records and traces as in the unsorted launch of one registration per workgroup."""
    check_sorted(mixed, 0, N_RAGGED, rpb)


@pytest.mark.gpu
def test_sorted_placement_beyond_one_stride_of_the_order_kernel(mixed):
    """1100 small registrations: the 1024 threads of k_solve_order take a second round"""
    check_sorted(mixed, N_RAGGED, N_MANY, 4)
