"""Raster scans (azimuth x range intensity rasters): the host-side definition the device entries are held to -- on the CPU."""
import numpy as np
import pytest

import pyoracle as po
from randt_slam_amd import host

from polar_raster_cases import SHAPES, filter_kw, speckle_and_ramps, tables


@pytest.mark.parametrize("dtype,scale", [(np.uint8, 1.0), (np.uint16, 0.5), (np.float32, 0.1)])
def test_expansion_is_the_definition(dtype, scale):
    """expand_polar_raster against a scalar loop of the definition: one float32 multiply per coordinate, z = 0,
    I = float32(v) * scale (the float32 raster is multiplied too)."""
    n_scans, n_az, n_bins = 2, 5, 37
    cossin, ranges = tables(n_scans, n_az, n_bins, seed=3)
    raster = speckle_and_ramps(11, n_scans, n_az, n_bins, dtype)
    if dtype == np.float32:
        raster = raster + np.float32(0.3)
    got = host.expand_polar_raster(raster, cossin, ranges, scale)
    assert got.dtype == np.float32 and got.shape == (n_scans, n_az, n_bins, 4)
    sc = np.float32(scale)
    for s in range(n_scans):
        for a in range(n_az):
            for b in range(n_bins):
                want = (np.float32(ranges[b]) * np.float32(cossin[s, a, 0]), np.float32(ranges[b]) * np.float32(cossin[s, a, 1]), np.float32(0.0),
                        np.float32(raster[s, a, b]) * sc)
                assert all(np.float32(g).tobytes() == np.float32(w).tobytes() for g, w in zip(got[s, a, b], want)), (s, a, b)
    # one table for all scans
    one = host.expand_polar_raster(raster, cossin[0], ranges, scale)
    assert np.array_equal(one[0].view(np.uint32), got[0].view(np.uint32))
    with pytest.raises(TypeError):
        host.expand_polar_raster(raster.astype(np.int32), cossin, ranges)


def test_polar_tables_round_once_from_double():
    az = np.array([0.1, 2.0, -3.0, np.pi, 1e-9, 0.5 * np.pi], dtype=np.float64)
    cossin, ranges = host.polar_tables(az, np.array([0.1, 0.2, 1.0 / 3.0]))
    assert cossin.dtype == np.float32 and cossin.shape == (6, 2) and ranges.dtype == np.float32
    import math
    for i, a in enumerate(az):
        assert cossin[i, 0] == np.float32(math.cos(float(a))) and cossin[i, 1] == np.float32(math.sin(float(a)))
    # not the float32 functions of a float32 angle: at 2.0 + 2^-30 the double result rounds differently from cosf(float(a))
    a = 2.0 + 2.0 ** -30
    assert host.polar_tables([a], [1.0])[0][0, 0] == np.float32(math.cos(a))
    assert ranges.tolist() == [np.float32(0.1), np.float32(0.2), np.float32(1.0 / 3.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d-%s" % (s[0], s[1], s[2], np.dtype(s[3]).name))
def test_the_tests_own_inputs_are_azimuth_organised_and_not_empty(built, shape):
    """Guards the inputs of the GPU tests: on every expansion the reference's azimuth detection (|atan2 - current| > 1e-4 while
    walking the cloud) finds exactly the rows -- n_az - 1 flushes, each with a detection --, and the first four shapes keep points."""
    n_scans, n_az, n_bins, dtype, _ = shape
    cossin, ranges = tables(n_scans, n_az, n_bins)
    raster = speckle_and_ramps(7, n_scans, n_az, n_bins, dtype)
    cloud = host.expand_polar_raster(raster, cossin, ranges)
    ofp = po.filter_params(**filter_kw(ranges))
    for s in range(n_scans):
        ang = np.arctan2(cloud[s, :, :, 1], cloud[s, :, :, 0]).astype(np.float32)
        assert (np.abs(ang - ang[:, :1]) <= 1e-4).all()                                # no azimuth change inside a row
        if n_az > 1:
            assert (np.abs(np.diff(ang[:, 0])) > 1e-4).all()                           # one between any two rows
        cnt, pts, pol, pk = po.filter_scan(cloud[s].reshape(-1, 4), ofp)
        assert len(pk) <= n_az - 1
        if shape in SHAPES[:4]:
            assert cnt > 0 and len(pk) == n_az - 1
            print(shape[:3], "scan", s, "keeps", cnt)


def test_host_raster_wants_one_2d_scan():
    for bad in (np.zeros(8, np.uint8), np.zeros((2, 3, 4), np.uint8)):
        with pytest.raises(ValueError):
            host._host_raster(bad)
    view = np.zeros((4, 20), np.uint8)[:, 11:]
    got, et, n_az, n_bins, pitch = host._host_raster(view)
    assert got is view and (et, n_az, n_bins, pitch) == (0, 4, 9, 20)
