"""-m gpu: the association's placements give the same correspondence tables, bit for bit.

A batch that shares the chip (RANDT_SOLVE_THROUGHPUT, more than 64 pairs) takes one workgroup per pair in the register-capped
instantiation; RANDT_ASSOC_TP_PPW=4 restores the older walk (one workgroup per four pairs, one after the other), and a lone batch
(RANDT_SOLVE_LATENCY) takes (pair, chunk) workgroups of the unconstrained instantiation.  Placement decides which
workgroup handles a cell, never which fixed cells it reads or in what order, so all three tables must agree -- on the config-4
batch bench.py times (512 pairs), on 65 pairs (just above the switch at 64) and on the wide (radius > 7) instantiation.
"""
import os

import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import synth
from util import GpuRig

pytestmark = pytest.mark.gpu

PLACEMENTS = {  # name: (environment at context creation, solve mode)
    "one_pair": ({}, R._capi.SOLVE_THROUGHPUT),
    "walk": ({"RANDT_ASSOC_TP_PPW": "4"}, R._capi.SOLVE_THROUGHPUT),
    "lone": ({}, R._capi.SOLVE_LATENCY),
}


def _ctx_with(torch, env, mode):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    ctx.set_solve_mode(mode)
    return ctx


@pytest.fixture(scope="module")
def cfg4(built):
    rig = GpuRig(synth.make_batch_problem(8, 64, 34))   # bench.py's base problem
    rig.build_submaps()
    rig.build_scans()
    return rig


def _tables(rig, n, mp):
    """Correspondence tables of the first n pairs of the batch under every placement (maps shared through storage views)."""
    torch = rig.torch
    guess = torch.from_numpy(synth.pose3_to_pose4(rig.prob["guess"][:n])).to(rig.dev)
    fidx = rig.fixed_idx[:n].contiguous()
    out = {}
    for name, (env, mode) in PLACEMENTS.items():
        ctx = _ctx_with(torch, env, mode)
        sub = R.Maps(ctx, rig.n_sub, rig.mapp, rig.mapp.size_x * rig.mapp.size_y, storage=rig.submaps.device_ptrs(), clear=False)
        scans = R.Maps(ctx, rig.B, rig.mapp, rig.scan_cap, storage=rig.scan_maps.device_ptrs(), clear=False)
        corr = torch.full((n, rig.scan_cap, mp.n_neighbours), -7, dtype=torch.int32, device=rig.dev)
        R.associate_batch(ctx, sub, fidx, scans, 0, n, guess, mp, corr)
        ctx.synchronize()
        out[name] = corr.cpu().numpy()
    return out


@pytest.mark.parametrize("n", [512, 65])
@pytest.mark.parametrize("mahal,intensity", [(1, 1), (0, 1)])
def test_placements_give_identical_tables(cfg4, n, mahal, intensity):
    rig = cfg4
    mp = R.default_matcher_params(lookup_mahalanobis=mahal, use_intensity=intensity)
    t = _tables(rig, n, mp)
    counts = rig.scan_maps.counts()[:n]
    assert (counts > 64).any()                      # some scans span several 64-cell chunks
    assert (t["one_pair"] >= 0).sum() > 10 * n      # real tables, not sentinels
    assert np.array_equal(t["one_pair"], t["walk"])
    assert np.array_equal(t["one_pair"], t["lone"])
    # nothing is written behind a scan's last cell
    for i in range(n):
        assert (t["one_pair"][i, counts[i]:] == -7).all(), i


def test_wide_window_identical_under_every_placement(built):
    """The wide instantiation (0.25 m cells with the 4 m window: radius 15; k = 12) with 70 copies of one pair: every placement
    and every copy gives the oracle's table."""
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(71)
    F = np.float32

    def blobs(n_blobs, n=2000):
        c = rng.uniform(-20.0, 20.0, (n_blobs, 2))
        pts = np.zeros((n, 4), dtype=F)
        pts[:, :2] = (c[rng.integers(0, n_blobs, n)] + rng.normal(0, 0.07, (n, 2))).astype(F)
        pts[:, 3] = rng.uniform(10, 90, n)
        return pts

    fixed_pts, moving_pts = blobs(60), blobs(40)
    mapp_args = (200, 200, 0.25, 0.0, 0.0, 4.0, 3, 0)
    mapp, clu = R.MapParams(*mapp_args), R.ClusterParams(2304, 24.0)
    k, n = 12, 70
    guess = np.tile(np.array([[np.cos(-0.04), np.sin(-0.04), 0.2, 0.25]]), (n, 1))
    mp = R.default_matcher_params(n_neighbours=k)
    got = {}
    for name, (env, mode) in PLACEMENTS.items():
        ctx = _ctx_with(torch, env, mode)
        fmap = R.Maps(ctx, 1, mapp, 4096, with_grid=True)
        mmap = R.Maps(ctx, n, mapp, 512, with_grid=False)
        R.ndt_build_batch(ctx, torch.from_numpy(fixed_pts[None]).to(dev), clu, fmap)
        R.ndt_build_batch(ctx, torch.from_numpy(np.broadcast_to(moving_pts, (n,) + moving_pts.shape).copy()).to(dev), clu, mmap)
        corr = torch.full((n, 512, k), -7, dtype=torch.int32, device=dev)
        R.associate_batch(ctx, fmap, torch.zeros(n, dtype=torch.int32, device=dev), mmap, 0, n, torch.from_numpy(guess).to(dev), mp, corr)
        ctx.synchronize()
        got[name] = corr.cpu().numpy()

    def omap(cap):
        return po.Map(mapp_args[0], mapp_args[1], mapp_args[2], (mapp_args[3], mapp_args[4]), mapp_args[5], mapp_args[6], cap)

    of, om = omap(4096), omap(512)
    of.build(fixed_pts, clu.n_clusters, clu.max_range)
    om.build(moving_pts, clu.n_clusters, clu.max_range)
    want, _ = po.associate(of, om, guess[0], k, 1, 1)
    assert om.n_cells > 5 and (want >= 0).sum() >= om.n_cells
    for name, t in got.items():
        for j in range(n):
            assert np.array_equal(t[j, : om.n_cells], want), (name, j)
