"""k_maps_merge / randt_maps_merge / randt_maps_merge_batch (mapops.hip) on moving maps of more than one 256-cell chunk.
Every other test merges scan maps of 45-101 cells, so the chunk loop runs once: the leader search that reaches back into
earlier chunks, followers in later chunks, the cell count carried from chunk to chunk and the capacity cut are never
exercised, and merge_batch is only seen through the lock-step odometry.

Moving maps: cells of several oracle scan maps built a metre apart and brought into one frame, in a seeded permuted order,
uploaded as they are (the oracle twin is Map.set).  Reference: the oracle's copy -> transform -> merge, map after map;
cells, cell count and index grid must come out bit for bit.  The unmarked tests pin the inputs on the oracle alone (which
slots collide across which chunks, where the capacity runs out), so they run without a GPU."""
import functools

import numpy as np
import pytest

import randt_slam_amd as R
from randt_slam_amd import synth
from util import cells_equal, oracle_map, oracle_scan_map

CHUNK = 256                                   # k_maps_merge walks the moving cells 256 at a time
N_SCANS = 14
POSE = synth.pose3_to_pose4([0.2, -0.1, 0.03])
POSES3 = synth.pose3_to_pose4(np.array([[0.2, -0.1, 0.03], [-0.35, 0.25, -0.05], [0.6, 0.4, 0.08]]))
SIZES = (255, 256, 257, 600)
N_SLOTS = 100 * 100


@functools.lru_cache(maxsize=None)
def scan_maps():
    """oracle maps of N_SCANS scans taken a metre apart, each moved into the frame of the first"""
    world = synth.make_world()
    tr = synth.make_trajectory(3000, N_SCANS, step=1.0)
    inv0 = synth.se2_inv3(tr[0])
    out = []
    for j in range(N_SCANS):
        m = oracle_scan_map(synth.make_scan(world, tr[j], 7000 + j))
        m.transform(synth.pose3_to_pose4(synth.se2_mul3(inv0, tr[j])))
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def pool(seed=11):
    cells = np.concatenate([m.cells() for m in scan_maps()])
    return cells[np.random.default_rng(seed).permutation(len(cells))]


@functools.lru_cache(maxsize=None)
def start(which=(0, 7, 13)):
    """a populated fixed map: (cells, grid) of the merge of some of the scan maps"""
    f = oracle_map()
    for j in which:
        f.merge(scan_maps()[j])
    return f.cells(), f.grid()


def twin(cells, cap=None):
    m = oracle_map(max(len(cells), 1) if cap is None else cap)
    m.set(cells, np.full(m.n_slots, -1, dtype=np.int32))
    return m


def reference(fc, fg, cap, movings):
    """the oracle's copy -> transform -> merge of every (cells, pose4), in order"""
    f = oracle_map(cap)
    f.set(fc, fg)
    for cells, pose in movings:
        m = twin(cells).copy()
        m.transform(pose)
        f.merge(m)
    return f


def slots_of(cells, pose):
    m = twin(cells)
    m.transform(pose)
    f = oracle_map(1)
    return np.array([f.coord_to_index(c["mean"][0], c["mean"][1]) for c in m.cells()], dtype=np.int64)


def walk(grid, n0, cap, slots):
    """what Map::mergeMapCell does with each cell, in order: 'o'utside the grid, 'm'erge, 'i'nsert, 'd'ropped for capacity"""
    have, n, out = set(np.flatnonzero(grid >= 0).tolist()), n0, []
    for s in slots:
        if s >= N_SLOTS:
            out.append("o")
        elif s in have:
            out.append("m")
        elif n < cap:
            have.add(s)
            n += 1
            out.append("i")
        else:
            out.append("d")
    return np.array(out), n


@functools.lru_cache(maxsize=None)
def moving_cells(M):
    """the first M cells of the pool; for 257 the one cell of the second chunk is the first later cell of the pool that falls
    into a slot which a cell of the first chunk newly inserts -- the shortest map with a follower in a later chunk"""
    if M != 257:
        return pool()[:M]
    fc, fg = start()
    s = slots_of(pool(), POSE)
    what, _ = walk(fg, len(fc), 10000, s[:256])
    new = set(s[:256][what == "i"].tolist())
    j = next(j for j in range(256, len(s)) if s[j] in new)
    return np.concatenate([pool()[:256], pool()[j:j + 1]])


def off_grid(cells, seed=31, n=70):
    """`cells` with a seeded tenth of them pushed 60 m up or down, out of the 50 m grid"""
    out = cells.copy()
    at = np.random.default_rng(seed).choice(len(cells), n, replace=False)
    out["mean"][at, 1] += np.where(np.arange(n) % 2 == 0, 60.0, -60.0).astype(np.float32)
    return out, np.sort(at)


def capacity_cases():
    """fixed capacities at which the 600-cell merge runs out of room inside chunk 0, with the last insert of chunk 0, and
    inside chunk 1"""
    fc, fg = start()
    what, _ = walk(fg, len(fc), 10000, slots_of(pool()[:600], POSE))
    ins = [int((what[c:c + CHUNK] == "i").sum()) for c in range(0, 600, CHUNK)]
    return {"inside chunk 0": len(fc) + ins[0] // 2, "at index 256": len(fc) + ins[0], "inside chunk 1": len(fc) + ins[0] + ins[1] // 2}


#            fixed map: starting scans, capacity;   moving maps: slices of two pools
BATCH_FIXED = (((0,), 300), ((1, 8), 300), ((2, 9, 12), 300), ((3,), 300), ((5, 6), 300))
BATCH = dict(fixed_first=1, n_fixed=3, moving_first=2, each=2, n_moving_maps=9)


def batch_moving(j):
    return pool(17)[37 * j:37 * j + (300, 180, 257, 40, 256, 120, 310, 90, 64)[j]]


def batch_poses():
    rng = np.random.default_rng(41)
    return synth.pose3_to_pose4(rng.normal(0, [0.3, 0.3, 0.05], (BATCH["n_fixed"] * BATCH["each"], 3)))


# ------------------------------------------------------------------ CPU: the inputs, on the oracle alone ----------
def test_collisions_span_the_chunks(built):
    fc, fg = start()
    assert len(pool()) > 700 and len(fc) > 100
    for M in SIZES:
        s = slots_of(moving_cells(M), POSE)
        what, n = walk(fg, len(fc), 10000, s)
        assert (s < N_SLOTS).all() and len(s) == M
        first = {}
        for i, v in enumerate(s.tolist()):
            first.setdefault(v, i)
        lead = np.array([first[v] for v in s.tolist()])                        # index of the cell that owns each cell's slot
        leaders = np.flatnonzero(lead == np.arange(M))
        per_chunk = [(int(((what[leaders] == "m") & (leaders // CHUNK == c)).sum()), int(((what[leaders] == "i") & (leaders // CHUNK == c)).sum()))
                     for c in range((M + CHUNK - 1) // CHUNK)]
        print("M", M, "distinct slots", len(first), "(merge, insert) leaders per chunk", per_chunk, "cells after", n)
        assert per_chunk[0][0] > 20 and per_chunk[0][1] > 20
        if M == 257:
            assert lead[256] < 256 and what[lead[256]] == "i" and what[256] == "m"      # a follower alone in its chunk
        if M == 600:
            assert all(m > 0 and i > 0 for m, i in per_chunk) and len(per_chunk) == 3   # both branches in every chunk
            n_of = {v: int((s == v).sum()) for v in first}
            spanning = [v for v, i0 in first.items() if i0 < 256 and (s[256:512] == v).any() and (s[512:] == v).any()]
            late = [v for v, i0 in first.items() if i0 >= 256 and n_of[v] > 1]
            print("slots led from chunk 0 with followers in chunks 1 and 2:", len(spanning), "led from a later chunk with followers:", len(late),
                  "hit three times or more:", sum(c >= 3 for c in n_of.values()))
            assert len(spanning) >= 5 and len(late) >= 5 and sum(c >= 3 for c in n_of.values()) >= 5
            assert any(first[v] >= 512 for v in first)                                  # the last chunk still finds new slots
    # the second and third map of the three-map merge bring their own cells
    assert len(pool()) >= 900


def test_off_grid_cells_are_interleaved(built):
    cells, at = off_grid(pool()[:600])
    s = slots_of(cells, POSE)
    out = np.flatnonzero(s >= N_SLOTS)
    assert np.array_equal(out, at) and len(at) == 70                    # both directions leave the grid, nothing wraps back into it
    assert all(((at // CHUNK) == c).sum() >= 5 for c in range(3)) and (np.diff(at) > 1).any()
    fc, fg = start()
    what, n = walk(fg, len(fc), 10000, s)
    assert (what[at] == "o").all() and (what == "i").sum() > 20 and (what == "m").sum() > 200
    assert reference(fc, fg, 10000, [(cells, POSE)]).n_cells == n


def test_capacity_runs_out_where_the_cases_say(built):
    fc, fg = start()
    s = slots_of(pool()[:600], POSE)
    for name, cap in capacity_cases().items():
        what, n = walk(fg, len(fc), cap, s)
        drop = np.flatnonzero(what == "d")
        last_insert = np.flatnonzero(what == "i").max()
        print(name, "capacity", cap, "first dropped cell", drop[0], "last insert", last_insert, "dropped", len(drop), "merges behind it", (what[drop[0]:] == "m").sum())
        assert n == cap and len(drop) > 0 and (what[drop[0]:] == "m").sum() > 50       # later cells still merge into existing slots
        if name == "inside chunk 0":
            assert 0 < drop[0] < CHUNK - 20 and (drop < CHUNK).sum() > 3 and (drop >= CHUNK).sum() > 3
        elif name == "at index 256":
            assert last_insert < CHUNK <= drop[0] and (what[:CHUNK] == "i").sum() == cap - len(fc)
        else:
            assert CHUNK < drop[0] < 2 * CHUNK and (drop >= 2 * CHUNK).sum() > 0
        # the second map of the same call meets a full map: it wants slots it cannot have, and merges into the others
        f = reference(fc, fg, cap, [(pool()[:600], POSE)])
        assert f.n_cells == cap == n
        what2, n2 = walk(f.grid(), cap, cap, slots_of(pool()[600:900], POSES3[1]))
        assert n2 == cap and (what2 == "d").sum() > 5 and (what2 == "m").sum() > 50


def test_batch_layout(built):
    b = BATCH
    assert b["fixed_first"] > 0 and b["moving_first"] > 0 and b["fixed_first"] + b["n_fixed"] < len(BATCH_FIXED)
    assert b["moving_first"] + b["n_fixed"] * b["each"] < b["n_moving_maps"]
    sizes = [len(batch_moving(j)) for j in range(b["n_moving_maps"])]
    used = sizes[b["moving_first"]:b["moving_first"] + b["n_fixed"] * b["each"]]
    assert max(used) > CHUNK and 256 in used and 257 in used and min(used) < 64
    for p in range(b["n_fixed"]):                                       # no merge of the batch runs out of room or leaves the grid
        which, cap = BATCH_FIXED[b["fixed_first"] + p]
        fc, fg = start(which)
        f = reference(fc, fg, cap, [(batch_moving(b["moving_first"] + p * b["each"] + t), batch_poses()[p * b["each"] + t]) for t in range(b["each"])])
        assert len(fc) < f.n_cells < cap


# ------------------------------------------------------------------ GPU ----------
class Rig:
    def __init__(self):
        import torch

        self.torch = torch
        self.ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
        self.mapp = R.indoor_map_params()

    def fixed(self, fc, fg, cap, ctx=None):
        fm = R.Maps(ctx or self.ctx, 1, self.mapp, cap, with_grid=True)
        fm.upload(0, fc, fg)
        return fm

    def moving(self, cell_arrays, mcap, ctx=None):
        mm = R.Maps(ctx or self.ctx, len(cell_arrays), self.mapp, mcap, with_grid=False)
        for j, c in enumerate(cell_arrays):
            mm.upload(j, c)
        return mm

    def merge(self, fc, fg, cap, movings, mcap=1024, ctx=None):
        """one randt_maps_merge call of every (cells, pose4) into the uploaded fixed map; (cells, count, grid) afterwards"""
        fm = self.fixed(fc, fg, cap, ctx)
        mm = self.moving([c for c, _ in movings], mcap, ctx)
        fm.merge(0, mm, 0, np.stack([p for _, p in movings]))
        cells, grid = fm.download(0)
        return cells, int(fm.counts()[0]), grid


@pytest.fixture(scope="module")
def rig(built):
    return Rig()


def check(got, ref, tag):
    cells, count, grid = got
    print("%s: %d cells, oracle %d" % (tag, count, ref.n_cells))
    assert count == ref.n_cells == len(cells), tag
    assert cells_equal(cells, ref.cells()), tag
    assert np.array_equal(grid, ref.grid()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("M", SIZES)
def test_chunk_boundaries_with_collisions(rig, M):
    """255 / 256 / 257 cells: the last chunk one short, full, one over (that one cell a follower of a cell inserted from chunk 0); 600: three chunks, slots led from chunk 0 with
    followers in chunks 1 and 2, leaders in later chunks with followers of their own, merges and inserts in every chunk."""
    fc, fg = start()
    movings = [(moving_cells(M), POSE)]
    check(rig.merge(fc, fg, 10000, movings), reference(fc, fg, 10000, movings), "M %d" % M)
    empty = np.full(N_SLOTS, -1, dtype=np.int32)                       # into an empty map: every leader inserts
    check(rig.merge(fc[:0], empty, 10000, movings), reference(fc[:0], empty, 10000, movings), "M %d into an empty map" % M)


@pytest.mark.gpu
def test_cells_outside_the_grid_are_skipped(rig):
    fc, fg = start()
    movings = [(off_grid(pool()[:600])[0], POSE)]
    check(rig.merge(fc, fg, 10000, movings), reference(fc, fg, 10000, movings), "off-grid cells")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["inside chunk 0", "at index 256", "inside chunk 1"])
def test_capacity_runs_out_inside_a_merge(rig, case):
    """the cut: inserts beyond the capacity are dropped with their followers, cells of later chunks still merge into the slots
    that exist, the count stops at the capacity -- and the second map of the same call sees that full map"""
    fc, fg = start()
    cap = capacity_cases()[case]
    one = [(pool()[:600], POSE)]
    check(rig.merge(fc, fg, cap, one), reference(fc, fg, cap, one), case)
    two = one + [(pool()[600:900], POSES3[1])]
    ref = reference(fc, fg, cap, two)
    assert ref.n_cells == cap
    check(rig.merge(fc, fg, cap, two), ref, case + ", two maps")


@pytest.mark.gpu
def test_three_moving_maps_with_distinct_poses(rig):
    fc, fg = start()
    movings = [(pool()[:600], POSES3[0]), (pool()[600:900], POSES3[1]), (pool()[300:700], POSES3[2])]
    ref = reference(fc, fg, 10000, movings)
    check(rig.merge(fc, fg, 10000, movings), ref, "three maps")
    same_pose = reference(fc, fg, 10000, [(c, POSES3[0]) for c, _ in movings])
    assert not np.array_equal(same_pose.grid(), ref.grid())           # the poses matter


@pytest.mark.gpu
def test_merge_batch_equals_single_merges_and_the_oracle(rig):
    """3 fixed x 2 moving maps in one launch, from fixed map 1 and moving map 2 on: what three randt_maps_merge calls give,
    what the oracle gives, and nothing on either side of the range is touched"""
    b = BATCH
    starts = [start(w) for w, _ in BATCH_FIXED]
    cap = BATCH_FIXED[0][1]
    fm = R.Maps(rig.ctx, len(BATCH_FIXED), rig.mapp, cap, with_grid=True)
    for j, (fc, fg) in enumerate(starts):
        fm.upload(j, fc, fg)
    single = fm.clone()
    mm = rig.moving([batch_moving(j) for j in range(b["n_moving_maps"])], 512)
    poses = batch_poses()
    fm.merge_batch(b["fixed_first"], b["n_fixed"], mm, b["moving_first"], poses)
    for p in range(b["n_fixed"]):
        single.merge(b["fixed_first"] + p, mm, b["moving_first"] + p * b["each"], poses[p * b["each"]:(p + 1) * b["each"]])
    counts, counts1 = fm.counts(), single.counts()
    for j, (fc, fg) in enumerate(starts):
        cells, grid = fm.download(j)
        cells1, grid1 = single.download(j)
        assert counts[j] == counts1[j] and cells_equal(cells, cells1) and np.array_equal(grid, grid1), j
        p = j - b["fixed_first"]
        if 0 <= p < b["n_fixed"]:
            first = b["moving_first"] + p * b["each"]
            ref = reference(fc, fg, cap, [(batch_moving(first + t), poses[p * b["each"] + t]) for t in range(b["each"])])
            check((cells, int(counts[j]), grid), ref, "batch, fixed map %d" % j)
        else:
            assert counts[j] == len(fc) and cells_equal(cells, fc) and np.array_equal(grid, fg), j
    for j in range(b["n_moving_maps"]):                                 # the moving maps are read only
        cells, _ = mm.download(j)
        assert cells_equal(cells, batch_moving(j)), j


@pytest.mark.gpu
def test_moving_capacity_beyond_48_kb_of_lds_and_the_refusal(built):
    """the slot list of the moving map lives in LDS, 4 B per cell of CAPACITY: 16000 cells need 64 KB, more than a kernel gets
    without asking (a new context, so the raise happens here); 65536 cells cannot fit the 160 KB and are refused, the fixed map
    untouched and the context usable; a fixed batch without an index grid is invalid."""
    import torch

    rig = Rig()
    assert rig.ctx is not None and torch.cuda.is_available()
    fc, fg = start()
    movings = [(pool()[:600], POSE)]
    ref = reference(fc, fg, 10000, movings)
    check(rig.merge(fc, fg, 10000, movings, mcap=16000), ref, "moving capacity 16000")
    fm = rig.fixed(fc, fg, 10000)
    big = rig.moving([pool()[:600]], 65536)
    with pytest.raises(R.RandtError) as e:
        fm.merge(0, big, 0, POSE[None])
    assert e.value.status == R._capi.ERR_UNSUPPORTED and "moving map capacity too large for merge kernel" in str(e.value)
    with pytest.raises(R.RandtError) as e:
        fm.merge_batch(0, 1, big, 0, POSE[None])
    assert e.value.status == R._capi.ERR_UNSUPPORTED
    cells, grid = fm.download(0)
    assert fm.counts()[0] == len(fc) and cells_equal(cells, fc) and np.array_equal(grid, fg)
    nogrid = R.Maps(rig.ctx, 1, rig.mapp, 10000, with_grid=False)
    nogrid.upload(0, fc)
    small = rig.moving([pool()[:600]], 1024)
    for call in (lambda: nogrid.merge(0, small, 0, POSE[None]), lambda: nogrid.merge_batch(0, 1, small, 0, POSE[None])):
        with pytest.raises(R.RandtError) as e:
            call()
        assert e.value.status == R._capi.ERR_INVALID
    fm.merge(0, small, 0, POSE[None])                                   # still alive, and right
    cells, grid = fm.download(0)
    check((cells, int(fm.counts()[0]), grid), ref, "after the refusals")
