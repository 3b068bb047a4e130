"""-m gpu: the scan filter on azimuth x range intensity rasters (randt_filter_raster*).  The raster entries must return what
the point-cloud entries return on the EXPANSION of the raster (host.expand_polar_raster), bit for bit: every comparison here
is made on the float bit patterns, against the existing device entry on the uploaded expansion AND against the CPU oracle's
filterScan on it.  (One exception, inherited from tests/test_filter.py: the oracle's atan2f is libm's, the device's is ocml's,
so the ANGLES are compared with the oracle to 1e-6 there as well; against the existing device entry they are bit-equal.)"""
import numpy as np
import pytest

import pyoracle as po
import randt_slam_amd as R
from randt_slam_amd import host, odometry, synth

from polar_raster_cases import BIN, SHAPES, bits, filter_kw, pitched_bytes, run_cloud, run_raster, speckle_and_ramps, tables

pytestmark = pytest.mark.gpu


def _ctx():
    import torch

    return R.Context(0, torch.cuda.current_stream().cuda_stream), torch.device("cuda:0")


def _same(res_r, res_c):
    """raster entry == cloud entry on the expansion: whole output buffers, status included"""
    for name, r, c in zip(("points", "polar", "peaks", "counts", "peak counts", "status"), res_r, res_c):
        assert np.array_equal(r.view(np.uint32), c.view(np.uint32)), name


def _oracle(res, cloud, ofp, clipped=None):
    out, polar, peaks, counts, pcounts, status = res
    total = 0
    for s in range(len(cloud)):
        cnt, pts, pol, pk = po.filter_scan(cloud[s].reshape(-1, 4), ofp)
        n = cnt if clipped is None else min(cnt, clipped)
        assert counts[s] == n and pcounts[s] == len(pk), s
        assert np.array_equal(bits(out[s, :n]), bits(pts[:n])), s
        assert np.array_equal(bits(polar[s, :n, 1]), bits(pol[:n, 1])), s
        assert np.allclose(polar[s, :n, 0], pol[:n, 0], atol=1e-6), s
        g = peaks[s, :len(pk)]
        assert np.array_equal(bits(g[:, 1:]), bits(pk[:, 1:])) and np.allclose(g[:, 0], pk[:, 0], atol=1e-6), s
        total += cnt
    return total


def _both(ctx, dev, raster, cossin, ranges, kw, scale=1.0, pitch=None, status=0):
    cloud = host.expand_polar_raster(raster, cossin, ranges, scale)
    fp, ofp = host.filter_params(**kw), po.filter_params(**kw)
    res_r = run_raster(ctx, dev, raster, cossin, ranges, fp, scale=scale, pitch=pitch)
    res_c = run_cloud(ctx, dev, cloud, fp)
    _same(res_r, res_c)
    assert res_r[5].tolist() == [status] * len(raster)
    return _oracle(res_r, cloud, ofp) if status == 0 else None


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d-%s" % (s[0], s[1], s[2], np.dtype(s[3]).name))
def test_raster_shapes(built, shape):
    n_scans, n_az, n_bins, dtype, pitch = shape
    ctx, dev = _ctx()
    cossin, ranges = tables(n_scans, n_az, n_bins)
    raster = speckle_and_ramps(7, n_scans, n_az, n_bins, dtype)
    scale = {np.uint8: 1.0, np.uint16: 0.5, np.float32: 0.75}[dtype]
    if dtype == np.uint16:
        raster = (raster.astype(np.int64) * 2 + 300 * (raster > 30)).astype(np.uint16)   # values beyond 8 bits
    total = _both(ctx, dev, raster, cossin, ranges, filter_kw(ranges), scale=scale, pitch=pitch)
    if shape in SHAPES[:4]:
        assert total > 0


def crafted_raster(n_az=16, n_bins=2100):
    """uint8 rows (three 16-byte loads of 1024 bins per wavefront: lane t of load u holds bins 1024 u + 16 t ..) whose runs take
    every road through the row kernel and the emission."""
    rng = np.random.default_rng(5)
    v = rng.integers(0, 5, (n_az, n_bins))

    def ramp(a, c, half, top, step=1):
        for d in range(-half, half + 1):
            j = a * n_bins + c + d
            if 0 <= j < n_az * n_bins:
                v[j // n_bins, j % n_bins] = top - step * abs(d)
    v[0] = 0                                              # azimuth 0 all zero: the first boundary still pushes index 0
    v[7] = 0                                              # an all-zero azimuth further on
    v[1, [35, 38]] = 120                                  # a tie between two bins of one lane (32 .. 47)
    v[2, [70, 300]] = 130                                 # between two lanes of one load
    v[3, [1500, 400]] = 140                               # between two loads
    v[3, 20], v[3, 150] = 90, 95                          # (the bins whose hypot the second parameter set uses as bounds)
    v[4, 500:520] = 150                                   # a plateau: the first of it is the detection, the walk stops at once
    ramp(4, 900, 6, 149)                                  # ... and it beats this ramp
    ramp(5, 1000, 80, 250)                                # 161 bins: far beyond the stage, several 32-bin steps on both sides
    ramp(6, 600, 1, 200, step=50)                         # at most 4 kept points: handed over ready-made
    v[8, 0], v[8, 1] = 180, 100                           # a detection in the first bin of a row
    v[9, n_bins - 1], v[9, n_bins - 2] = 190, 100         # ... and in the last
    ramp(11, 0, 5, 210, step=7)                           # a ramp at a row start: with min_range below ranges[0] the inward
    #                                                       walk crosses into azimuth 10's last bins
    ramp(12, 1023, 3, 220, step=9)                        # a run across a load boundary
    ramp(14, 2050, 2, 230, step=20)
    v[15, 100] = 255                                      # the last azimuth is never flushed
    return v.astype(np.uint8)[None]


def test_raster_crafted_runs(built):
    ctx, dev = _ctx()
    raster = crafted_raster()
    _, n_az, n_bins = raster.shape
    cossin, ranges = tables(1, n_az, n_bins, seed=1)
    total = _both(ctx, dev, raster, cossin, ranges, filter_kw(ranges, min_range=0.01))
    assert total > 161 + 20
    # default-like thresholds: runs end at once towards the sensor when the bin spacing exceeds the threshold
    assert _both(ctx, dev, raster, cossin, ranges, filter_kw(ranges, beam_thr=0.04)) > 0
    # min_range / max_range exactly the hypot of a bin of azimuth 3 (strict comparisons: both bins are out)
    cloud = host.expand_polar_raster(raster, cossin, ranges)[0]
    hyp = lambda a, b: float(np.float32(np.sqrt(float(cloud[a, b, 0]) ** 2 + float(cloud[a, b, 1]) ** 2)))
    kw = filter_kw(ranges, min_range=hyp(3, 20), max_range=hyp(3, 150))
    assert _both(ctx, dev, raster, cossin, ranges, kw) > 0
    only3 = raster.copy()
    only3[0, 3] = 0
    only3[0, 3, 20], only3[0, 3, 150], only3[0, 3, 100] = 90, 95, 50      # the two bound bins are the strongest, and excluded
    cnt, pts, pol, pk = po.filter_scan(host.expand_polar_raster(only3, cossin, ranges)[0].reshape(-1, 4), po.filter_params(**kw))
    assert pk[[abs(p[2] - 50.0) < 1e-6 for p in pk]].shape[0] == 1 and not any(p[2] in (90.0, 95.0) for p in pk)
    _both(ctx, dev, only3, cossin, ranges, kw)


def test_raster_tables_and_padding(built):
    """Padding bytes of 255 (run_raster's default) in a pitched row, a batch whose scans have different cossin tables, rows at
    the +-pi cut (s = +0.0 and s = -8.7e-8: the exact atan2f walk), a sensor->base transform with a non-zero T10."""
    ctx, dev = _ctx()
    n_scans, n_az, n_bins = 3, 11, 300
    cossin, ranges = tables(n_scans, n_az, n_bins, seed=2)
    assert not np.array_equal(cossin[0], cossin[1])
    cossin[0, 4] = (-1.0, 0.0)
    cossin[1, 4] = (-1.0, -8.7e-8)
    cossin[2, 0] = (-1.0, -8.7e-8)
    raster = speckle_and_ramps(21, n_scans, n_az, n_bins, np.uint8)
    c, s_ = np.cos(0.3), np.sin(0.3)
    T = np.array([[c, -s_, 0.1, 0.3], [s_, c, -0.2, -0.7], [0.05, 0.02, 1.5, 1.5]], dtype=np.float32)
    kw = filter_kw(ranges, sensor_to_base=T)
    assert _both(ctx, dev, raster, cossin, ranges, kw, pitch=320) > 0
    # the padding never wins: were it looked at, 255 would be every row's detection
    fp = host.filter_params(**kw)
    a = run_raster(ctx, dev, raster, cossin, ranges, fp, pitch=320, pad=255)
    b = run_raster(ctx, dev, raster, cossin, ranges, fp, pitch=304, pad=0)
    _same(a, b)
    # uint16 with a scale, the same tables
    r16 = (raster.astype(np.uint16) * 257)
    assert _both(ctx, dev, r16, cossin, ranges, filter_kw(ranges, sensor_to_base=T, min_intensity=6.0), scale=1.0 / 257.0, pitch=608) > 0


def test_raster_status(built):
    import torch

    ctx, dev = _ctx()
    n_scans, n_az, n_bins = 2, 12, 200
    cossin, ranges = tables(n_scans, n_az, n_bins, seed=4)
    raster = speckle_and_ramps(31, n_scans, n_az, n_bins, np.uint8)
    kw = filter_kw(ranges)
    fp, ofp = host.filter_params(**kw), po.filter_params(**kw)
    cloud = host.expand_polar_raster(raster, cossin, ranges)
    # output overflow: status 2, the first pitch_out points
    res_r = run_raster(ctx, dev, raster, cossin, ranges, fp, pitch_out=8)
    _same(res_r, run_cloud(ctx, dev, cloud, fp, pitch_out=8))
    assert res_r[5].tolist() == [2, 2] and res_r[3].tolist() == [8, 8]
    _oracle(res_r, cloud, ofp, clipped=8)
    # a duplicated azimuth: two consecutive rows closer than 1e-4 rad
    dup = cossin.copy()
    dup[1, 6] = dup[1, 5]
    res_r = run_raster(ctx, dev, raster, dup, ranges, fp)
    _same(res_r, run_cloud(ctx, dev, host.expand_polar_raster(raster, dup, ranges), fp))
    assert res_r[5].tolist() == [0, 1]
    # a non-positive range: the zero-length point's atan2(0, 0) = 0 starts an azimuth of its own
    zr = ranges.copy()
    zr[0] = 0.0
    res_r = run_raster(ctx, dev, raster, cossin, zr, fp)
    _same(res_r, run_cloud(ctx, dev, host.expand_polar_raster(raster, cossin, zr), fp))
    assert res_r[5].tolist() == [1, 1]
    # a device raster that is not 16-byte aligned, or a row pitch that is not: RANDT_ERR_INVALID, outputs untouched
    buf = torch.zeros(n_scans * n_az * 208 + 16, dtype=torch.uint8, device=dev)
    out = torch.full((n_scans, 64, 4), 7.0, dtype=torch.float32, device=dev)
    counts = torch.full((n_scans,), -3, dtype=torch.int32, device=dev)
    status = torch.full((n_scans,), -5, dtype=torch.int32, device=dev)
    d_cs, d_rg = torch.from_numpy(cossin).to(dev), torch.from_numpy(ranges).to(dev)
    for ptr, pitch in ((buf.data_ptr() + 1, 208), (buf.data_ptr() + 8, 208), (buf.data_ptr(), 204)):
        desc = host.polar_raster_desc(0, n_az, n_bins, pitch)
        with pytest.raises(host.RandtError) as e:
            host.filter_raster_batch(ctx, ptr, desc, d_cs, d_rg, n_scans, fp, out, counts, status)
        assert e.value.status == 1 and "16" in str(e.value)
    ctx.synchronize()
    assert (out == 7.0).all().item() and counts.cpu().tolist() == [-3, -3] and status.cpu().tolist() == [-5, -5]


def test_raster_host_entries(built):
    """randt_filter_raster from a buffer with an 11-byte header per row (pitch n_bins + 11: nothing aligned), and
    randt_filter_raster_build against randt_filter_build on the expansion."""
    ctx, dev = _ctx()
    n_az, n_bins = 40, 501
    cossin, ranges = tables(1, n_az, n_bins, seed=6)
    raster = speckle_and_ramps(41, 1, n_az, n_bins, np.uint8)[0]
    image = np.full((n_az, n_bins + 11), 255, dtype=np.uint8)       # what an Oxford radar PNG row looks like: metadata, then values
    image[:, 11:] = raster
    view = image[:, 11:]
    assert view.strides == (n_bins + 11, 1) and not view.flags["C_CONTIGUOUS"]
    kw = filter_kw(ranges)
    fp, ofp = host.filter_params(**kw), po.filter_params(**kw)
    cloud = host.expand_polar_raster(raster, cossin[0], ranges)
    cnt, pts, pol, pk = po.filter_scan(cloud.reshape(-1, 4), ofp)
    assert cnt > 40
    g_pts, g_pol, g_pk, n, status = host.filter_raster_host(ctx, view, cossin[0], ranges, fp, capacity=2048)
    assert status == 0 and n == cnt and len(g_pk) == len(pk)
    assert np.array_equal(bits(g_pts), bits(pts)) and np.array_equal(bits(g_pol[:, 1]), bits(pol[:, 1])) and np.allclose(g_pol[:, 0], pol[:, 0], atol=1e-6)
    assert np.array_equal(bits(g_pk[:, 1:]), bits(pk[:, 1:])) and np.allclose(g_pk[:, 0], pk[:, 0], atol=1e-6)
    # ... and bit for bit what the point-cloud twin returns on the expansion, angles included
    c_pts, c_pol, c_pk, c_n, c_status = host.filter_scan_host(ctx, cloud, fp, capacity=2048)
    assert (c_n, c_status) == (n, status) and all(np.array_equal(bits(a), bits(b)) for a, b in ((g_pts, c_pts), (g_pol, c_pol), (g_pk, c_pk)))
    g3, _, _, n3, st3 = host.filter_raster_host(ctx, view, cossin[0], ranges, fp, capacity=16, want_polar=False, want_peaks=False)
    assert st3 == 2 and n3 == 16 and np.array_equal(bits(g3), bits(pts[:16]))
    # uint16 from an odd start address
    raw16 = np.zeros(n_az * (2 * n_bins + 6) + 1, dtype=np.uint8)
    v16 = np.ndarray((n_az, n_bins), dtype=np.uint16, buffer=raw16.data, offset=1, strides=(2 * n_bins + 6, 2))
    v16[:] = raster.astype(np.uint16) * 200
    g16 = host.filter_raster_host(ctx, v16, cossin[0], ranges, fp, scale=1.0 / 200.0, capacity=2048)
    c16 = host.filter_scan_host(ctx, host.expand_polar_raster(np.ascontiguousarray(v16), cossin[0], ranges, 1.0 / 200.0), fp, capacity=2048)
    assert g16[3:] == c16[3:] and g16[3] > 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(g16[:3], c16[:3]))
    # filter -> clustering -> NDT, on a scene whose returns are dense enough to form cells
    rasters, cs2, rg2, fp2 = _drive_scene(1)
    view2 = np.full((rasters[0].shape[0], rasters[0].shape[1] + 11), 255, dtype=np.uint8)
    view2[:, 11:] = rasters[0]
    cloud2 = host.expand_polar_raster(rasters[0], cs2, rg2)
    maps = R.Maps(ctx, 2, R.indoor_map_params(), 1024, with_grid=True)
    clu = R.indoor_cluster_params()
    assert host.filter_build(ctx, cloud2, fp2, clu, maps, 0) == 0
    assert host.filter_raster_build(ctx, view2[:, 11:], cs2, rg2, fp2, clu, maps, 1) == 0
    (c0, g0), (c1, g1) = maps.download(0), maps.download(1)
    from util import cells_equal, oracle_scan_map
    om = oracle_scan_map(po.filter_scan(cloud2.reshape(-1, 4), po.filter_params(beam_thr=0.3))[1], cap=1024)
    assert len(c0) > 20 and cells_equal(c0, c1) and np.array_equal(g0, g1)
    assert cells_equal(c1, om.cells()) and np.array_equal(g1, om.grid())
    assert host.filter_raster_build(ctx, view2[:, 11:], cs2, rg2, fp2, clu, maps, 0, wait=False) is None
    assert cells_equal(maps.download(0)[0], c1)


def _drive_scene(n_scans, n_az=200, n_bins=600):
    """synth's room seen as uint8 rasters: make_polar_scan's intensities quantised, its azimuths and bins as tables"""
    world = synth.make_world()
    traj = synth.make_trajectory(3500, n_scans, step=0.25)
    bin_size = 0.0438 * 5
    az = -np.pi + (np.arange(n_az) + 0.5) * (2 * np.pi / n_az)
    cossin, ranges = host.polar_tables(az, (np.arange(n_bins) + 0.5) * bin_size)
    rasters = [np.clip(np.rint(synth.make_polar_scan(world, traj[i], 11000 + i, n_az=n_az, n_bins=n_bins, bin_size=bin_size)[..., 3]), 0, 255).astype(np.uint8)
               for i in range(n_scans)]
    return rasters, cossin, ranges, host.filter_params(beam_thr=0.3)


def test_raster_odometry_drive(built):
    """process_scan(..., polar_raster=...) over 6 scans = the same drive fed the expansions: poses bit-equal."""
    import torch

    n_scans, dt = 6, 0.25
    rasters, cossin, ranges, fp = _drive_scene(n_scans)
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    wp = R.window_params()

    def drive(raster_path):
        ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
        odo = odometry.Odometry(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params()), mp, wp)
        poses = []
        for i in range(n_scans):
            if raster_path:
                poses.append(odo.process_scan(rasters[i], i * dt, polar_filter=fp, polar_raster=(cossin, ranges, 1.0)).copy())
            else:
                poses.append(odo.process_scan(host.expand_polar_raster(rasters[i], cossin, ranges), i * dt, polar_filter=fp).copy())
            assert int(odo.b._f_cnt.cpu()[0]) > 100 and int(odo.b._f_status.cpu()[0]) == 0
        return np.array(poses)
    a, b = drive(True), drive(False)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.abs(a[-1] - a[0]).max() > 0.1                       # the drive moved
