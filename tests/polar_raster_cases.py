"""Inputs and runners shared by the raster-filter tests (test_filter_raster_host.py on the CPU, test_gpu_filter_raster.py on the
GPU): scans delivered as azimuth x range intensity rasters, their tables, and the two device paths held to each other."""
import numpy as np

from randt_slam_amd import host

# (n_scans, n_az, n_bins, dtype, row pitch in bytes): baseline, padded row, more than one round of loads per wavefront
# (4096 uint8 bins are one round), uint16, float32, degenerate
SHAPES = [
    (1, 12, 80, np.uint8, 80),
    (3, 7, 300, np.uint8, 304),
    (2, 16, 4200, np.uint8, 4208),
    (2, 9, 130, np.uint16, 272),
    (1, 5, 63, np.float32, 256),
    (1, 2, 1, np.uint8, 16),
]
BIN = 0.16                                   # metres per bin: below beam_thr 0.2, so runs grow towards the sensor too
FILTER_KW = dict(min_range=0.6, min_intensity=6.0, beam_thr=0.2)


def tables(n_scans, n_az, n_bins, seed=0):
    """Distinct azimuths per scan (each scan of a batch gets its own offset: its own cossin table) and ascending ranges."""
    rng = np.random.default_rng(1000 + seed)
    az = -np.pi + (np.arange(n_az) + 0.5) * (2 * np.pi / n_az)
    az = az[None] + rng.uniform(-0.2, 0.2, (n_scans, 1)) / n_az
    cossin = np.stack([host.polar_tables(az[s], [1.0])[0] for s in range(n_scans)])
    ranges = host.polar_tables([0.0], (np.arange(n_bins) + 0.5) * BIN)[1]
    return cossin, ranges


def speckle_and_ramps(seed, n_scans, n_az, n_bins, dtype):
    """Speckle below min_intensity plus two planted ramps per azimuth (integers, so every element type holds them exactly)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 5, (n_scans, n_az, n_bins))
    for s in range(n_scans):
        for a in range(n_az):
            for top in rng.integers(40, 200, 2):
                c, half = int(rng.integers(0, n_bins)), int(rng.integers(1, 4))
                for d in range(-half, half + 1):
                    if 0 <= c + d < n_bins:
                        v[s, a, c + d] = max(v[s, a, c + d], top - 9 * abs(d))
    return v.astype(dtype)


def filter_kw(ranges, **over):
    kw = dict(FILTER_KW, max_range=float(ranges[-1]) + 1.0)
    kw.update(over)
    return kw


def pitched_bytes(raster, pitch, pad=255):
    """(n_scans, n_az, pitch) uint8: the rows of `raster` at a row pitch of `pitch` bytes, every padding byte = pad."""
    n_scans, n_az, n_bins = raster.shape
    row = n_bins * raster.itemsize
    buf = np.full((n_scans, n_az, pitch), pad, dtype=np.uint8)
    buf[:, :, :row] = np.ascontiguousarray(raster).view(np.uint8).reshape(n_scans, n_az, row)
    return buf


def _outputs(torch, dev, n_scans, n_az, pitch_out):
    return (torch.zeros((n_scans, pitch_out, 4), dtype=torch.float32, device=dev), torch.zeros((n_scans, pitch_out, 2), dtype=torch.float32, device=dev),
            torch.zeros((n_scans, n_az, 3), dtype=torch.float32, device=dev), torch.zeros(n_scans, dtype=torch.int32, device=dev),
            torch.zeros(n_scans, dtype=torch.int32, device=dev), torch.zeros(n_scans, dtype=torch.int32, device=dev))


def _host(ctx, outs):
    ctx.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def run_raster(ctx, dev, raster, cossin, ranges, fp, scale=1.0, pitch=None, pad=255, pitch_out=4096):
    """randt_filter_raster_batch_dev -> (points, polar, peaks, counts, peak counts, status) on the host, whole buffers."""
    import torch

    n_scans, n_az, n_bins = raster.shape
    pitch = pitch or ((n_bins * raster.itemsize + 15) & ~15)
    d_ras = torch.from_numpy(pitched_bytes(raster, pitch, pad)).to(dev)
    desc = host.polar_raster_desc(host._RASTER_TYPES[raster.dtype], n_az, n_bins, pitch, scale=scale)
    out, polar, peaks, counts, pcounts, status = outs = _outputs(torch, dev, n_scans, n_az, pitch_out)
    host.filter_raster_batch(ctx, d_ras, desc, torch.from_numpy(np.ascontiguousarray(cossin)).to(dev), torch.from_numpy(ranges).to(dev), n_scans, fp,
                             out, counts, status, polar, peaks, pcounts)
    return _host(ctx, outs)


def run_cloud(ctx, dev, cloud, fp, pitch_out=4096):
    """The existing point-cloud entry on an expansion, same outputs."""
    import torch

    n_scans, n_az = cloud.shape[:2]
    out, polar, peaks, counts, pcounts, status = outs = _outputs(torch, dev, n_scans, n_az, pitch_out)
    host.filter_scan_batch(ctx, torch.from_numpy(cloud).to(dev), fp, out, counts, status, polar, peaks, pcounts)
    return _host(ctx, outs)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
