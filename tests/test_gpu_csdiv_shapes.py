"""SURVEY row f-2 beyond the default shapes: k_cs_self / k_cs_pair (csdiv.hip) at their tile edges, with empty and all-invalid
maps, window offsets, no pose, moving maps up to the LDS limit (the triangle decode above 2^24 / 8 items) and the refusal
beyond it.  Reference: the CPU oracle (same fp32 pair terms, sequential fp64 sums); one multi-tile case against the float64
numpy definition of csdiv_ref.py.  The unmarked tests pin the oracle itself, so they run without a GPU."""
import functools

import numpy as np
import pytest

import csdiv_ref
import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import host, synth
from util import oracle_map

CELL = R.CELL_DTYPE
CAP = 1024
# k_cs_self: 16 outer cells per workgroup, inner cells staged 256 at a time; k_cs_pair: 256-cell tiles of the fixed map
FIXED_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1000)
#                 moving count, fixed map of the batch call, fixed map of the second pairing
PAIRS = ((1000, 11, 2), (512, 0, 8), (513, 3, 8), (511, 7, 2), (3, 5, 11), (1000, 5, 0), (2, 4, 10), (512, 6, 1),
         (0, 7, 9), (1, 9, 5), (513, 9, 3), (511, 10, 4), (3, 1, 6), (2, 11, 7), (1000, 9, 2), (512, 10, 8))
WINDOW = dict(fixed_first=3, fixed_count=5, moving_first=2, n_pairs=7)     # pairs 2..8 use fixed maps 3..7 only
FAR_POSE = np.array([1.0, 0.0, 1.0e4, -1.0e4])                             # carries a moving map out of every fixed cell's reach


def omap(cells):
    m = oracle_map(max(len(cells), 1))
    m.set(cells, np.full(m.n_slots, -1, dtype=np.int32))
    return m


def oracle_cs(fc, mc, pose4=None):
    m = omap(mc)
    if pose4 is not None:
        m.transform(pose4)
    return po.cs_divergence(omap(fc), m)


@functools.lru_cache(maxsize=None)
def tile_maps():
    """Case 1: every fixed count once, 16 moving maps clustered on the fixed map they meet in the batch call."""
    rng = np.random.default_rng(4101)
    fixed = [csdiv_ref.rand_cells(rng, n, CELL) for n in FIXED_COUNTS]
    moving = [csdiv_ref.rand_cells(rng, n, CELL, centres=fixed[f]["mean"]) for n, f, _ in PAIRS]
    return fixed, moving


@functools.lru_cache(maxsize=None)
def tile_ref(pairing):
    """Oracle (value, terms) of the 16 pairs; pairing 1 = the batch call's, 2 = the second one's."""
    fixed, moving = tile_maps()
    return [oracle_cs(fixed[p[pairing]], moving[i]) for i, p in enumerate(PAIRS)]


def check_pair(out, terms, ref_v, ref_t, nf, nm, tag):
    """The issue's bars: terms at max(1e-10, 2 n_addends 2^-53) relative (the worst case of reordering a sum of non-negative
    terms; above 1e-10 only for millions of pairs), an exact zero where the oracle has one, the divergence at 1e-10 and of the
    oracle's class (NaN / +-inf) where a term is zero."""
    print("%s: terms %r oracle %r | cs %r oracle %r" % (tag, terms.tolist(), ref_t.tolist(), float(out), ref_v))
    for e, n_add in enumerate((nf * nm, nf * (nf + 1) // 2, nm * (nm + 1) // 2)):
        if ref_t[e] == 0.0:
            assert terms[e] == 0.0, (tag, e, terms[e])
        else:
            rtol = max(1e-10, 2.0 * n_add * 2.0 ** -53)
            assert abs(terms[e] - ref_t[e]) <= rtol * abs(ref_t[e]), (tag, e, terms[e], ref_t[e], rtol)
    assert np.isnan(out) == np.isnan(ref_v) and np.isposinf(out) == np.isposinf(ref_v) and np.isneginf(out) == np.isneginf(ref_v), (tag, out, ref_v)
    assert np.isclose(out, ref_v, rtol=1e-10, atol=1e-10, equal_nan=True), (tag, out, ref_v)


# ------------------------------------------------------------------ CPU: the oracle and the recipe ----------
def test_recipe_layout():
    fixed, moving = tile_maps()
    assert [len(c) for c in fixed] == list(FIXED_COUNTS)
    assert sorted(set(p[0] for p in PAIRS)) == [0, 1, 2, 3, 511, 512, 513, 1000]
    used = [set(p[col] for p in PAIRS) for col in (1, 2)]
    assert len(used[0]) < len(FIXED_COUNTS) < len(PAIRS)                      # repeats, and fixed maps the batch call never asks for
    assert used[0] | used[1] == set(range(len(FIXED_COUNTS)))                 # ... which the second pairing reads
    w = WINDOW
    for p in PAIRS[w["moving_first"]:w["moving_first"] + w["n_pairs"]]:
        assert w["fixed_first"] <= p[1] < w["fixed_first"] + w["fixed_count"]   # anything else reads outside the partial sums
    for c in fixed + moving:
        v = csdiv_ref.valid_cells(c)                       # (asserts the 5 % margin around the gate)
        assert not v[::7].any() and (len(c) < 2 or v[1:7].all())


def test_oracle_empty_and_all_invalid_maps(built):
    """0 cells, or only cells under the det(S) gate (the recipe's cell 0 is one): zero terms; NaN where the interaction term is
    among them (inf - inf), -inf where only the moving map's own term is."""
    fixed, moving = tile_maps()
    full_f, full_m = fixed[5], moving[2]
    for fc, mc, zero in ((fixed[0], full_m, (0, 1)), (fixed[1], full_m, (0, 1)), (full_f, moving[8], (0, 2)), (full_f, moving[9], (2,)),
                         (fixed[0], moving[8], (0, 1, 2)), (fixed[1], moving[9], (0, 1, 2))):
        v, t = oracle_cs(fc, mc)
        assert all(t[e] == 0.0 for e in zero) and all(t[e] > 0.0 for e in range(3) if e not in zero), (len(fc), len(mc), v, t)
        assert np.isnan(v) if 0 in zero else np.isneginf(v), (len(fc), len(mc), v, t)


def test_oracle_far_pose_gives_plus_infinity(built):
    """every pair term underflows to exactly 0: -log(0) with positive self terms"""
    fixed, moving = tile_maps()
    v, t = oracle_cs(fixed[5], moving[4], FAR_POSE)
    assert t[0] == 0.0 and t[1] > 0 and t[2] > 0 and np.isposinf(v)


@functools.lru_cache(maxsize=None)
def definition_case():
    rng = np.random.default_rng(4105)
    fc = csdiv_ref.rand_cells(rng, 300, CELL)
    return fc, csdiv_ref.rand_cells(rng, 600, CELL, centres=fc["mean"])


def test_oracle_matches_numpy_definition_multi_tile(built):
    """Case 5 on the CPU: 300 x 600 cells, the oracle's fp32 pair terms against float64.  Measured: interaction 1.2e-5,
    self terms 7.9e-5 and 3.2e-4 relative, divergence 1.1e-4 absolute -- inside the 3e-5 / 3e-3 of the 60 x 50 test."""
    fc, mc = definition_case()
    ref, ref_t = csdiv_ref.cs_definition(fc, mc)
    v, t = oracle_cs(fc, mc)
    print("oracle vs definition: rel", np.abs(t / ref_t - 1.0), "abs", abs(v - ref))
    assert np.isclose(t[0], ref_t[0], rtol=3e-5) and np.allclose(t[1:], ref_t[1:], rtol=3e-3)
    assert np.isclose(v, ref, rtol=0, atol=3e-3)
    assert ref_t[0] > 1e-3 * np.sqrt(ref_t[1] * ref_t[2])      # the clustering keeps the interaction term in play


# ------------------------------------------------------------------ GPU ----------
class Rig:
    def __init__(self):
        import torch

        self.torch, self.dev = torch, torch.device("cuda:0")
        self.ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
        self.mapp = R.indoor_map_params()
        fixed, moving = tile_maps()
        self.fm = self.upload(fixed, CAP, True)
        self.mm = self.upload(moving, CAP, False)
        self.out1, self.terms1 = self.batch(self.fm, 0, len(fixed), [p[1] for p in PAIRS], self.mm, 0, len(PAIRS), None)

    def upload(self, cell_arrays, cap, with_grid):
        maps = R.Maps(self.ctx, len(cell_arrays), self.mapp, cap, with_grid=with_grid)
        for i, c in enumerate(cell_arrays):
            maps.upload(i, c)
        if with_grid:
            maps.reindex()
        return maps

    def batch(self, fm, fixed_first, fixed_count, fixed_idx, mm, moving_first, n_pairs, poses4, want_terms=True):
        torch = self.torch
        out = torch.full((n_pairs,), -7.0, dtype=torch.float64, device=self.dev)
        terms = torch.full((n_pairs, 3), -7.0, dtype=torch.float64, device=self.dev) if want_terms else None
        fidx = torch.tensor(list(fixed_idx), dtype=torch.int32, device=self.dev)
        pose = None if poses4 is None else torch.from_numpy(np.ascontiguousarray(poses4, dtype=np.float64)).to(self.dev)
        host.cs_divergence_batch(self.ctx, fm, fixed_first, fixed_count, fidx, mm, moving_first, n_pairs, pose, out, terms)
        self.ctx.synchronize()
        return out.cpu().numpy(), (terms.cpu().numpy() if want_terms else None)


@pytest.fixture(scope="module")
def rig(built):
    return Rig()


@pytest.mark.gpu
@pytest.mark.parametrize("pairing", [1, 2])
def test_tile_edges_ragged_batch(rig, pairing):
    """Case 1.  pairing 1: the batch call every other test refers to; 2: the same maps met differently, so that every fixed
    count (k_cs_self: 15 / 16 / 17 outer cells, 255 / 256 / 257 and 511 / 512 / 513 inner) is read by some pair."""
    fixed, _ = tile_maps()
    if pairing == 1:
        out, terms = rig.out1, rig.terms1
    else:
        out, terms = rig.batch(rig.fm, 0, len(fixed), [p[2] for p in PAIRS], rig.mm, 0, len(PAIRS), None)
    ref = tile_ref(pairing)
    for i, p in enumerate(PAIRS):
        check_pair(out[i], terms[i], ref[i][0], ref[i][1], FIXED_COUNTS[p[pairing]], p[0], "pair %d (%d x %d)" % (i, FIXED_COUNTS[p[pairing]], p[0]))
    assert sum(np.isnan(r[0]) for r in ref) >= 3 and any(np.isneginf(r[0]) for r in ref) and sum(np.isfinite(r[0]) for r in ref) >= 8


@pytest.mark.gpu
def test_offsets_equal_the_whole_batch_bit_for_bit(rig):
    """Case 2: fixed_first = 3, fixed_count = 5, moving_first = 2 -- the `fmap - fixed_first` row of the partial sums."""
    w = WINDOW
    lo = w["moving_first"]
    fidx = [p[1] for p in PAIRS[lo:lo + w["n_pairs"]]]
    out, terms = rig.batch(rig.fm, w["fixed_first"], w["fixed_count"], fidx, rig.mm, lo, w["n_pairs"], None)
    assert np.array_equal(out, rig.out1[lo:lo + w["n_pairs"]], equal_nan=True)
    assert np.array_equal(terms, rig.terms1[lo:lo + w["n_pairs"]])
    for j in range(w["n_pairs"]):
        v1, t1 = host.cs_divergence(rig.ctx, rig.fm, fidx[j], rig.mm, lo + j)
        assert np.array_equal(np.array(v1), out[j], equal_nan=True) and np.array_equal(t1, terms[j]), (j, v1, out[j], t1, terms[j])
    # without the terms output the divergence is the same
    out_only, _ = rig.batch(rig.fm, w["fixed_first"], w["fixed_count"], fidx, rig.mm, lo, w["n_pairs"], None, want_terms=False)
    assert np.array_equal(out_only, out, equal_nan=True)


@pytest.mark.gpu
def test_no_pose_and_a_pose_per_pair(rig):
    """Case 3: d_pose4 = NULL is the untransformed map (test_tile_edges_ragged_batch compares that call with the oracle; here:
    an identity pose gives the same bits); a different pose per pair equals the oracle on the transformed copy, a pose that
    carries the map out of reach gives the oracle's +inf."""
    fixed, moving = tile_maps()
    n = len(PAIRS)
    ident = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    out, terms = rig.batch(rig.fm, 0, len(fixed), [p[1] for p in PAIRS], rig.mm, 0, n, ident)
    ref = tile_ref(1)
    for i, p in enumerate(PAIRS):
        check_pair(out[i], terms[i], ref[i][0], ref[i][1], FIXED_COUNTS[p[1]], p[0], "identity, pair %d" % i)
    rng = np.random.default_rng(4103)
    poses = synth.pose3_to_pose4(rng.normal(0, [0.15, 0.15, 0.05], (n, 3)))
    poses[4] = FAR_POSE
    poses[6, :2] *= 1.3                                          # not normalised: pose_to_affine_f divides by the length
    out, terms = rig.batch(rig.fm, 0, len(fixed), [p[1] for p in PAIRS], rig.mm, 0, n, poses)
    for i, p in enumerate(PAIRS):
        v, t = oracle_cs(fixed[p[1]], moving[i], poses[i])
        check_pair(out[i], terms[i], v, t, FIXED_COUNTS[p[1]], p[0], "posed, pair %d" % i)
        if i not in (4, 6) and np.isfinite(v):
            assert not np.isclose(v, ref[i][0], rtol=1e-6)      # the pose was applied
    assert np.isposinf(out[4])
    v1, t1 = host.cs_divergence(rig.ctx, rig.fm, PAIRS[5][1], rig.mm, 5, poses[5])
    assert v1 == out[5] and np.array_equal(t1, terms[5])


LARGE_CAP = 3700          # 148 000 B of dynamic LDS: the largest the entry admits is (160 KB - 12 KB) / 40 B = 3788 cells
LARGE = ((300, 2048), (300, 2049), (300, 3700), (3000, 300))   # 2048: the first triangle above 2^24 / 8 items; 3700: 6.8 M pairs


@functools.lru_cache(maxsize=None)
def large_maps():
    rng = np.random.default_rng(4104)
    fixed = [csdiv_ref.rand_cells(rng, 300, CELL), csdiv_ref.rand_cells(rng, 3000, CELL)]
    moving = [csdiv_ref.rand_cells(rng, nm, CELL, centres=fixed[nf == 3000]["mean"]) for nf, nm in LARGE]
    return fixed, moving


@pytest.fixture(scope="module")
def large(rig):
    fixed, moving = large_maps()
    fm = rig.upload(fixed, 3000, True)
    mm = rig.upload(moving, LARGE_CAP, False)
    return rig.batch(fm, 0, 2, [int(nf == 3000) for nf, _ in LARGE], mm, 0, len(LARGE), None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LARGE)), ids=["%dx%d" % c for c in LARGE])
def test_large_moving_maps(large, case):
    """Case 4: the sqrtf triangle decode where its float argument is no longer exact, more than 64 KB of dynamic LDS, and
    188 self-term tiles x 12 fixed tiles."""
    fixed, moving = large_maps()
    nf, nm = LARGE[case]
    v, t = oracle_cs(fixed[nf == 3000], moving[case])
    assert np.isfinite(v) and t.min() > 0
    check_pair(large[0][case], large[1][case], v, t, nf, nm, "%d x %d" % (nf, nm))


@pytest.mark.gpu
def test_numpy_definition_multi_tile(rig):
    """Case 5: 300 x 600 cells against float64 numpy, at the tolerances of test_cs_divergence_vs_numpy_definition (the oracle's
    own distance from the definition is measured in test_oracle_matches_numpy_definition_multi_tile)."""
    fc, mc = definition_case()
    ref, ref_t = csdiv_ref.cs_definition(fc, mc)
    fm, mm = rig.upload([fc], 300, True), rig.upload([mc], 600, False)
    out, terms = rig.batch(fm, 0, 1, [0], mm, 0, 1, None)
    print("device vs definition: rel", np.abs(terms[0] / ref_t - 1.0), "abs", abs(out[0] - ref))
    assert np.isclose(terms[0, 0], ref_t[0], rtol=3e-5), (terms, ref_t)
    assert np.allclose(terms[0, 1:], ref_t[1:], rtol=3e-3), (terms, ref_t)
    assert np.isclose(out[0], ref, rtol=0, atol=3e-3)


@pytest.mark.gpu
def test_capacity_refusal_leaves_the_context_usable(rig):
    """Case 6: 4096 x 40 B + 12 KB does not fit the 160 KB of LDS."""
    fixed, moving = tile_maps()
    big = R.Maps(rig.ctx, 1, rig.mapp, 4096, with_grid=False)
    big.upload(0, moving[0])
    with pytest.raises(R.RandtError) as e:
        rig.batch(rig.fm, 0, len(fixed), [11], big, 0, 1, None)
    assert e.value.status == R._capi.ERR_UNSUPPORTED and "moving-map capacity too large for the CS-divergence kernel" in str(e.value)
    with pytest.raises(R.RandtError) as e:
        host.cs_divergence(rig.ctx, rig.fm, 11, big, 0)
    assert e.value.status == R._capi.ERR_UNSUPPORTED
    out, terms = rig.batch(rig.fm, 0, len(fixed), [p[1] for p in PAIRS], rig.mm, 0, len(PAIRS), None)
    assert np.array_equal(out, rig.out1, equal_nan=True) and np.array_equal(terms, rig.terms1)


@pytest.mark.gpu
def test_two_calls_are_bit_identical(rig):
    """Case 7: fixed-order reductions."""
    fixed, _ = tile_maps()
    for _ in range(2):
        out, terms = rig.batch(rig.fm, 0, len(fixed), [p[1] for p in PAIRS], rig.mm, 0, len(PAIRS), None)
        assert np.array_equal(out, rig.out1, equal_nan=True) and np.array_equal(terms, rig.terms1)
