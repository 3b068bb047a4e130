#!/usr/bin/env python3
"""Time randt_pose_graph_covariance next to ONE randt_pose_graph_optimize call on the full-size graph of
tests/test_posegraph.py::test_hip_pose_graph_full_size_properties (2200 nodes, 60 loop closures, noisy version).

    python tools/posegraph_cov_probe.py [--runs 9] [--warmup 2]
        event-timed on the context's stream after a warm-up, median of --runs; one JSON line.  Both calls are host-synchronous
        (uploads, launches, one read-back), so the events bracket what a caller waits for.
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/posegraph_cov_probe.py --profile
        one warm call and one measured call of each, optimise first, for the per-kernel split (no counters in that run);
    python tools/posegraph_cov_probe.py --split DIR
        reads DIR/**/run_kernel_stats.csv and prints the k_pg_* rows: the k_pg_cov_* kernels run in the covariance call
        only; the others are shared with the optimiser's iterations.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def full_size_graph():
    from posegraph_cov_ref import make_graph

    n = 2200
    rng = np.random.default_rng(21)
    loops = [(int(a), int(a) + 1100 + int(o)) for a, o in zip(rng.integers(0, 1000, 60), rng.integers(-40, 40, 60))]
    _, x0, ia, ib, meas, sq = make_graph(n, loops, seed=23, laps=2.0, radius=60.0)
    return n, x0, ia, ib, meas, sq


def split(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if r.get("Name", "").find("k_pg_") >= 0:
                    rows.append(r)
    if not rows:
        print("no k_pg_* rows under", directory)
        return 1
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    for r in rows:
        name = r["Name"][r["Name"].find("k_pg_"):].split("(")[0]
        print("%-24s calls %5d total %9.1f us average %8.2f us" % (name, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--split", metavar="DIR")
    a = ap.parse_args()
    if a.split:
        return split(a.split)
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import host

    runs, warmup = (1, 1) if a.profile else (a.runs, a.warmup)
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    n, x0, ia, ib, meas, sq = full_size_graph()

    def timed(fn):
        ms = []
        for k in range(warmup + runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                ms.append(e0.elapsed_time(e1))
        return out, float(np.median(ms)), ms

    (x1, res), opt_ms, opt_all = timed(lambda: host.pose_graph_optimize(ctx, x0, ia, ib, meas, sq, n))
    cov, cov_ms, cov_all = timed(lambda: host.pose_graph_covariance(ctx, x1, ia, ib, meas, sq, n, None, -1))
    print(json.dumps({
        "graph": {"poses": n, "edges": int(len(ia)), "separator_poses": res["n_separator_poses"]},
        "optimize_ms_median": opt_ms, "optimize_iterations": res["iterations"], "optimize_ms_per_iteration": opt_ms / res["iterations"],
        "covariance_ms_median": cov_ms, "covariance_over_one_iteration": cov_ms / (opt_ms / res["iterations"]),
        "covariance_over_optimize": cov_ms / opt_ms, "runs": runs, "warmup": warmup,
        "optimize_ms_all": opt_all, "covariance_ms_all": cov_all,
        "largest_position_sigma_m": float(np.sqrt(max(c[0, 0] + c[1, 1] for c in cov))),
    }))
    return 0


if __name__ == "__main__":
    sys.exit(main())
