"""-m gpu: the host side's scratch storage -- the grow-only workspace, the pinned window image, the named words of the small
block and the pooled temporaries -- at the sizes the other tests do not reach: results must not depend on what a context's
buffers held before, on which entry point ran before, or on a buffer having been grown in between.  No oracle: every check is
bit-equality between two ways of running the same calls."""
import numpy as np
import pytest

import randt_slam_amd as R
from randt_slam_amd import host as H
from randt_slam_amd import synth

pytestmark = pytest.mark.gpu


def _ctx():
    import torch

    return R.Context(0, torch.cuda.current_stream().cuda_stream)


def _cells(rng, n, centre=(0.0, 0.0), spread=3.0):
    """n random cells with symmetric positive definite covariances."""
    c = np.zeros(n, dtype=R.CELL_DTYPE)
    c["mean"][:, :2] = rng.normal(0, spread, (n, 2)) + centre
    c["mean"][:, 2] = rng.uniform(5, 60, n)
    A = rng.normal(0, 0.3, (n, 3, 3))
    cov = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(3)
    c["cov"] = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], axis=1)
    c["n"] = rng.integers(6, 60, n)
    c["max_intensity"] = c["mean"][:, 2] + rng.uniform(0, 10, n)
    return c


def test_elementwise_entries_survive_regrowth():
    """cells_merge, cells_transform, cells_mahalanobis and points_transform with 3, then 20 000, then 3 elements on ONE context (the
    workspace grows in between; 20 000 points at stride 8 = 640 KB do not fit a 512 KB segment of the pinned ring): the entries
    work element by element, so the large result equals the same input pushed through in chunks of 257 on a fresh context, and
    the two small calls equal each other."""
    rng = np.random.default_rng(11)
    N, CH = 20000, 257
    a, b = _cells(rng, N), _cells(rng, N)
    pts = rng.normal(0, 4, (N, 8)).astype(np.float32)
    pose = np.array([np.cos(0.4), np.sin(0.4), 1.5, -0.75])
    ops = {
        "cells_merge": (lambda c, s: H.cells_merge(c, a[s], b[s])),
        "cells_transform": (lambda c, s: H.cells_transform(c, a[s], pose)),
        "cells_mahalanobis": (lambda c, s: H.cells_mahalanobis(c, a[s], b[s])),
        "points_transform": (lambda c, s: H.points_transform(c, pts[s], pose)),
    }
    one, other = _ctx(), _ctx()
    for name, op in ops.items():
        small0 = op(one, slice(0, 3))
        large = op(one, slice(0, N))
        small1 = op(one, slice(0, 3))
        assert small0.tobytes() == small1.tobytes(), name
        assert large[:3].tobytes() == small0.tobytes(), name
        chunks = np.concatenate([op(other, slice(i, min(i + CH, N))) for i in range(0, N, CH)])
        assert chunks.shape == large.shape and chunks.tobytes() == large.tobytes(), name
    grown = one.pool_stats()
    assert grown["device_allocs"] >= 2 and grown["device_frees"] >= 1      # the workspace really was replaced by a larger one


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_scene():
    """A 20 x 20-slot map of capacity 64 with some cells in it, a second map to register against it, and the inputs of the five
    host-level calls -- as host arrays, so that every context starts from an identical copy."""
    import torch

    ctx = _ctx()
    ip = synth.indoor_params()
    mapp = R.MapParams(20, 20, 0.5, 0.0, 0.0, ip["max_neighbour_dist"], ip["min_points_per_cell"], 0)
    clu = R.ClusterParams(400, 5.0)
    world = synth.make_world()
    traj = synth.make_trajectory(3000, 3)
    scans = []
    for i in range(2):
        s = synth.make_scan(world, traj[i], 500 + i, n_az=120)
        s[:, :2] *= 0.3                                   # the 12 m of a scan into the map's +-5 m
        scans.append(s)
    built = R.Maps(ctx, 2, mapp, 64, with_grid=True)
    R.ndt_build_batch(ctx, torch.from_numpy(np.stack(scans)).cuda(), clu, built)
    fixed, moving = built.download(0), built.download(1)
    assert 10 < len(fixed[0]) < 56 and len(moving[0]) > 10
    rng = np.random.default_rng(5)
    cluster = np.zeros((30, 4), dtype=np.float32)
    cluster[:, :2] = rng.normal(0, 0.08, (30, 2)) + [3.9, -4.1]
    cluster[:, 3] = rng.uniform(10, 40, 30)
    return dict(mapp=mapp, fixed=fixed, moving=moving, cluster=cluster, cells=_cells(rng, 3, spread=1.5), queries=_cells(rng, 5, spread=1.5),
                guess=synth.pose3_to_pose4(np.array([0.05, -0.04, 0.01])), mp=R.default_matcher_params())


def _maps(ctx, sc, fixed):
    """fresh copies of the scene's two maps on ctx; `fixed` = (cells, grid) the fixed one starts from"""
    f = R.Maps(ctx, 1, sc["mapp"], 64, with_grid=True)
    f.upload(0, *fixed)
    m = R.Maps(ctx, 1, sc["mapp"], 64, with_grid=False)
    m.upload(0, sc["moving"][0])
    return f, m


_CALLS = {
    "insert_cluster": lambda ctx, sc, f, m: f.insert_cluster(0, sc["cluster"]),
    "register_pair": lambda ctx, sc, f, m: H.register_pair(ctx, f, 0, m, 0, sc["mp"], sc["guess"]),
    "cs_divergence": lambda ctx, sc, f, m: H.cs_divergence(ctx, f, 0, m, 0, sc["guess"]),
    "insert_cells": lambda ctx, sc, f, m: f.insert_cells(0, sc["cells"], set_grid=True),
    "closest_cells": lambda ctx, sc, f, m: f.closest_cells(0, sc["queries"], k=4),
}


def _sequence(ctx, sc, f, m):
    """the five calls back to back, nothing of the test's own in between; then the map"""
    f.upload(0, *sc["fixed"])
    out = {name: call(ctx, sc, f, m) for name, call in _CALLS.items()}
    out["map"] = f.download(0)
    return out


def _blob(v):
    """every output as bytes: bools, floats, arrays and tuples of them"""
    if isinstance(v, (tuple, list)):
        return b"|".join(_blob(x) for x in v)
    return np.asarray(v).tobytes()


def test_nested_host_entries_do_not_share_slots(small_scene):
    """insert_cluster (which builds, then appends), register_pair, cs_divergence (both call batch entries that use the workspace),
    insert_cells and closest_cells (pooled temporaries) in sequence on ONE context give, bit for bit, what each gives as the only
    call of a fresh context on an identical copy of the map."""
    sc = small_scene
    ctx = _ctx()
    got = _sequence(ctx, sc, *_maps(ctx, sc, sc["fixed"]))
    assert got["insert_cluster"] is True and got["register_pair"][1]["n_residuals"] > 0 and np.isfinite(got["cs_divergence"][0])
    assert (got["closest_cells"] >= 0).any()
    state = sc["fixed"]                                   # what the fixed map holds in front of each call
    for name, call in _CALLS.items():
        alone = _ctx()
        f, m = _maps(alone, sc, state)
        want = call(alone, sc, f, m)
        assert _blob(want) == _blob(got[name]), name
        state = f.download(0)
    assert len(state[0]) > len(sc["fixed"][0])
    assert _blob(state) == _blob(got["map"])


def test_steady_state_makes_no_allocator_calls(small_scene):
    """The same sequence twice: the second run finds every buffer grown and every temporary parked -- no hipMalloc, no hipFree --
    and gives the same outputs."""
    sc = small_scene
    ctx = _ctx()
    f, m = _maps(ctx, sc, sc["fixed"])
    first = _sequence(ctx, sc, f, m)
    s0 = ctx.pool_stats()
    second = _sequence(ctx, sc, f, m)
    s1 = ctx.pool_stats()
    assert s1["device_allocs"] == s0["device_allocs"] and s1["device_frees"] == s0["device_frees"], (s0, s1)
    assert s1["pool_hits"] > s0["pool_hits"]
    for name in first:
        assert _blob(first[name]) == _blob(second[name]), name


def test_window_image_regrows():
    """register_window_batch with 1, then 9, then 1 windows (lag 2, one fixed map, scans of 200 points): the pinned image and the
    workspace grow in between; the first and third call agree bit for bit, and so does window 0 of the nine."""
    import torch

    ctx = _ctx()
    mapp, clu = R.indoor_map_params(), R.indoor_cluster_params()
    world = synth.make_world()
    traj = synth.make_trajectory(3100, 16, step=0.25)
    inv = synth.se2_inv3(traj[0])
    rel = np.array([synth.se2_mul3(inv, p) for p in traj])
    rel[:, 2] = synth.wrap_angle(rel[:, 2])
    kf = np.stack([synth.make_scan(world, traj[t], 7000 + t) for t in range(0, 4)])
    scans = np.stack([synth.make_scan(world, traj[4 + i], 8000 + i, n_az=40) for i in range(11)])
    assert scans.shape[1] == 200
    sub = R.Maps(ctx, 1, mapp, 4096, with_grid=True)
    tmp = R.Maps(ctx, len(kf), mapp, 512, with_grid=False)
    R.ndt_build_batch(ctx, torch.from_numpy(kf).cuda(), clu, tmp)
    sub.merge(0, tmp, 0, synth.pose3_to_pose4(rel[0:4]))
    smaps = R.Maps(ctx, len(scans), mapp, 128, with_grid=False)
    R.ndt_build_batch(ctx, torch.from_numpy(scans).cuda(), clu, smaps)
    W, S, dt = 9, 2, 0.25
    truth = rel[4:]
    states = np.zeros((W, S + 1), dtype=R.STATE_DTYPE)
    midx = np.zeros((W, S), dtype=np.int32)
    for w in range(W):
        st = R.make_state(synth.pose3_to_pose4(truth[w] + [0.02, -0.015, 0.003]), lin_vel=(0.8, 0.0), stamp=w * dt)
        states[w, 0] = st
        for j in range(1, S + 1):
            st = R.predict_state(st, (w + j) * dt)
            states[w, j] = st
            midx[w, j - 1] = w + j
    trans = np.stack([states[w, S]["pose"] for w in range(W)])
    fidx = np.zeros((W, 1), dtype=np.int32)
    mp, wp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3), R.window_params()

    def run(n):
        return R.register_window_batch(ctx, sub, fidx[:n], smaps, midx[:n], states[:n], mp, wp, trans[:n])

    first, nine, third = run(1), run(W), run(1)
    assert first[3]["n_residuals"][0] > 10 and first[3]["iterations"][0] >= 1
    for a, b, c in zip(first, nine, third):
        assert a.tobytes() == c.tobytes()
        assert a[0].tobytes() == b[0].tobytes()
    assert len({nine[0][w].tobytes() for w in range(W)}) == W            # nine different problems
