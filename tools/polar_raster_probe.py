"""The scan filter on raster scans against the point-cloud entry on the expansion of the same rasters.

Scene: Navtech-shaped scans, 400 azimuths x 3768 uint8 bins at a row pitch of 3776 bytes (1.5 MB per scan; the expansion is
24.1 MB).  Three configurations, the baseline of each being the existing point-cloud entry on the expansion:

  device-resident, 1 scan per launch      randt_filter_raster_batch_dev   vs  randt_filter_scan_batch_dev
  device-resident, 16 scans per launch    randt_filter_raster_batch_dev   vs  randt_filter_scan_batch_dev
  from a fresh pageable host buffer       randt_filter_raster_build       vs  randt_filter_build

Device-resident figures are HIP-event times over a window of launches that rotate over distinct input buffers (so that no
launch meets its own lines in the caches); the window is enqueued behind a few milliseconds of unrelated device work, so that
it measures the device and not the host's enqueue rate (one scan per launch is about as long as its two enqueues).  Host figures are a host clock around the synchronous call on a newly allocated buffer.
Every figure is the median of --reps samples with its spread (max - min) / median; the two sides of a line are sampled
alternately.  The outputs of both sides are compared bit for bit at the probed size before anything is timed.

  python tools/polar_raster_probe.py [--reps 7] [--out FILE]
  python tools/polar_raster_probe.py --baseline-only --lib other/librandt_hip.so     # the existing entry of another build
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_AZ, N_BINS, PITCH = 400, 3768, 3776
BIN = 0.0438


def make_rasters(n, seed):
    """n uint8 scans of a square room (walls 8 m from a sensor that sits a little off-centre, differently in every scan):
    speckle below the intensity gate and a five-bin return where each azimuth meets a wall."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 6, (n, N_AZ, N_BINS), dtype=np.uint8)
    prof = np.array([30, 60, 90, 60, 30], dtype=np.uint8)
    az = -np.pi + (np.arange(N_AZ) + 0.5) * (2 * np.pi / N_AZ)
    off = rng.uniform(-1.5, 1.5, (n, 2, 1))
    cx, cy = np.cos(az)[None], np.sin(az)[None]
    r = np.minimum((8.0 - np.sign(cx) * off[:, 0]) / np.maximum(np.abs(cx), 1e-9), (8.0 - np.sign(cy) * off[:, 1]) / np.maximum(np.abs(cy), 1e-9))
    c = np.clip(np.floor(r / BIN).astype(np.int64), 20, 270)  # inside max_range 12 m = 274 bins
    for k in range(5):
        np.put_along_axis(v, (c + k - 2)[..., None], prof[k] + rng.integers(0, 20, (n, N_AZ, 1), dtype=np.uint8), axis=2)
    return v


def stats(samples):
    s = sorted(samples)
    med = s[len(s) // 2]
    return {"median_us": round(med, 3), "min_us": round(s[0], 3), "max_us": round(s[-1], 3), "spread": round((s[-1] - s[0]) / med, 4), "samples": len(s)}


def verdict(raster, base):
    gain = 1.0 - raster["median_us"] / base["median_us"]
    need = max(0.10, raster["spread"], base["spread"])
    return {"gain": round(gain, 4), "needed": round(need, 4), "speedup": round(base["median_us"] / raster["median_us"], 3), "beats_baseline": bool(gain > need)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=48, help="launches per timed window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of librandt_hip.so")
    ap.add_argument("--baseline-only", action="store_true", help="only the point-cloud entry at 16 scans per launch (works with builds that lack the raster entries)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    import torch

    import randt_slam_amd as R
    from randt_slam_amd import _capi, host

    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.baseline_only:
        for name in [k for k in _capi.SYMBOLS if "raster" in k]:
            del _capi.SYMBOLS[name]
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    fp = host.filter_params()
    az = -np.pi + (np.arange(N_AZ) + 0.5) * (2 * np.pi / N_AZ)
    cossin, ranges = host.polar_tables(az, (np.arange(N_BINS) + 0.5) * BIN)
    d_rg = torch.from_numpy(ranges).to(dev)

    def device_inputs(n_scans, n_sets, seed):
        """n_sets distinct batches: the pitched rasters, their tables and their expansions (formed on the device with the
        definition's single float32 multiplies)."""
        sets = []
        for k in range(n_sets):
            v = make_rasters(n_scans, seed + k)
            buf = np.full((n_scans, N_AZ, PITCH), 255, dtype=np.uint8)
            buf[:, :, :N_BINS] = v
            d_ras = torch.from_numpy(buf).to(dev)
            d_cs = torch.from_numpy(np.broadcast_to(cossin, (n_scans, N_AZ, 2)).copy()).to(dev)
            cloud = torch.zeros((n_scans, N_AZ, N_BINS, 4), dtype=torch.float32, device=dev)
            cloud[..., 0] = d_rg[None, None, :] * d_cs[:, :, 0:1]
            cloud[..., 1] = d_rg[None, None, :] * d_cs[:, :, 1:2]
            cloud[..., 3] = d_ras[:, :, :N_BINS].to(torch.float32)
            sets.append((d_ras, d_cs, cloud))
        return sets

    def outputs(n_scans, pitch_out=8192):
        return (torch.zeros((n_scans, pitch_out, 4), dtype=torch.float32, device=dev), torch.zeros(n_scans, dtype=torch.int32, device=dev),
                torch.zeros(n_scans, dtype=torch.int32, device=dev))

    blocker = torch.randn((8192, 8192), dtype=torch.float32, device=dev)

    def window(fn, n_sets, launches):
        """one sample: microseconds per launch over a window of launches rotating over the input sets"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            torch.mm(blocker, blocker)                              # the host gets ahead of the device while this runs
        e0.record()
        for i in range(launches):
            fn(i % n_sets)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    result = {"scene": {"n_azimuths": N_AZ, "n_bins": N_BINS, "row_pitch_bytes": PITCH, "raster_bytes_per_scan": N_AZ * PITCH,
                        "cloud_bytes_per_scan": N_AZ * N_BINS * 16}, "reps": args.reps}
    desc = None if args.baseline_only else host.polar_raster_desc(_capi.RASTER_U8, N_AZ, N_BINS, PITCH)
    for n_scans, n_sets in ((1, 16), (16, 4)):
        if args.baseline_only and n_scans == 1:
            continue
        sets = device_inputs(n_scans, n_sets, 100 * n_scans)
        out_r, cnt_r, st_r = outputs(n_scans)
        out_c, cnt_c, st_c = outputs(n_scans)

        def run_raster(k):
            host.filter_raster_batch(ctx, sets[k][0], desc, sets[k][1], d_rg, n_scans, fp, out_r, cnt_r, st_r)

        def run_cloud(k):
            host.filter_scan_batch(ctx, sets[k][2], fp, out_c, cnt_c, st_c)
        run_cloud(0)
        key = "device_%d_scan%s_per_launch" % (n_scans, "" if n_scans == 1 else "s")
        if not args.baseline_only:
            run_raster(0)
            ctx.synchronize()
            assert st_r.cpu().tolist() == [0] * n_scans == st_c.cpu().tolist() and int(cnt_r.sum()) > 400 * n_scans
            assert torch.equal(cnt_r, cnt_c) and torch.equal(out_r.view(torch.int32), out_c.view(torch.int32)), "raster and cloud paths differ"
        launches = args.launches * (8 if n_scans == 1 else 1)
        for _ in range(2):                                          # warm-up of both shapes
            window(run_cloud, n_sets, launches)
            if not args.baseline_only:
                window(run_raster, n_sets, launches)
        r_s, c_s = [], []
        for _ in range(args.reps):
            if not args.baseline_only:
                r_s.append(window(run_raster, n_sets, launches))
            c_s.append(window(run_cloud, n_sets, launches))
        result[key] = {"launches_per_window": launches, "baseline_cloud": stats(c_s)}
        if not args.baseline_only:
            result[key]["raster"] = stats(r_s)
            result[key]["verdict"] = verdict(result[key]["raster"], result[key]["baseline_cloud"])
        del sets
    if not args.baseline_only:
        # one scan from a fresh pageable host buffer -> filter -> clustering -> NDT, the call waited for
        maps = R.Maps(ctx, 2, R.indoor_map_params(), 1024, with_grid=True)
        clu = R.indoor_cluster_params()
        v = make_rasters(1, 7)[0]
        image = np.full((N_AZ, PITCH), 255, dtype=np.uint8)
        image[:, :N_BINS] = v
        cloud = host.expand_polar_raster(v, cossin, ranges)

        def host_raster():
            fresh = image.copy()                                   # a new pageable allocation, as a sensor callback's buffer
            t = time.perf_counter()
            st = host.filter_raster_build(ctx, fresh[:, :N_BINS], cossin, ranges, fp, clu, maps, 0)
            return (time.perf_counter() - t) * 1e6, st

        def host_cloud():
            fresh = cloud.copy()
            t = time.perf_counter()
            st = host.filter_build(ctx, fresh, fp, clu, maps, 1)
            return (time.perf_counter() - t) * 1e6, st
        for _ in range(3):
            assert host_raster()[1] == 0 and host_cloud()[1] == 0
        (c0, g0), (c1, g1) = maps.download(0), maps.download(1)
        same = len(c0) == len(c1) and all(np.array_equal(c0[f].view(np.uint32), c1[f].view(np.uint32)) for f in ("mean", "cov", "n", "max_intensity"))
        assert len(c0) > 50, "the probe's scene forms too few cells: %d" % len(c0)
        assert same and np.array_equal(g0, g1), "raster and cloud builds differ"
        r_s, c_s = [], []
        for _ in range(max(args.reps, 9)):
            r_s.append(host_raster()[0])
            c_s.append(host_cloud()[0])
        result["host_fresh_pageable_build"] = {"raster": stats(r_s), "baseline_cloud": stats(c_s)}
        result["host_fresh_pageable_build"]["verdict"] = verdict(stats(r_s), stats(c_s))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
