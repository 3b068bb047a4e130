"""-m gpu: raster scans through the C++ facade (tests/cpp/polar_raster_drive.cpp): RadarPreprocessor::filterPolarRaster /
processPolarRaster and LocalFuser::processPolarRaster equal the point-cloud overloads on the expansions of the same rasters."""
import os
import subprocess

import numpy as np
import pytest

from randt_slam_amd import host, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "randt-slam_amd")


def _build(tmp_path):
    exe = str(tmp_path / "polar_raster_drive")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "polar_raster_drive.cpp"),
        "-L", LIBDIR, "-lrandt_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe,
    ])
    return exe


def test_cpp_raster_overloads_equal_the_cloud_overloads_on_the_expansions(built, tmp_path):
    world = synth.make_world()
    n_scans, n_az, n_bins = 4, 200, 600
    bin_size = 0.0438 * 5
    traj = synth.make_trajectory(3500, n_scans, step=0.25)
    az = -np.pi + (np.arange(n_az) + 0.5) * (2 * np.pi / n_az)
    cossin, ranges = host.polar_tables(az, (np.arange(n_bins) + 0.5) * bin_size)
    rasters = np.stack([np.clip(np.rint(synth.make_polar_scan(world, traj[i], 11000 + i, n_az=n_az, n_bins=n_bins, bin_size=bin_size)[..., 3]), 0, 255)
                        for i in range(n_scans)]).astype(np.uint8)
    path = tmp_path / "rasters.bin"
    with open(path, "wb") as f:
        f.write(np.array([n_scans, n_az, n_bins], dtype=np.int32).tobytes())
        f.write(np.array([1.0], dtype=np.float32).tobytes())
        f.write(cossin.tobytes())
        f.write(ranges.tobytes())
        f.write(rasters.tobytes())
    exe = _build(tmp_path)
    for extra in ([], ["--slam"]):
        r = subprocess.run([exe, str(path)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "DIFFERENT" not in r.stdout and r.stdout.count(": equal") == 5, r.stdout
