#!/usr/bin/env python3
"""N correlative searches as a loop of randt_search_global calls against ONE randt_search_global_batch_dev call, on the config-4
scene (8 submaps, 512 scans; pair p = scan p against its submap from truth + (0.9, -0.7, 0.1), cost threshold 2.0, the default
windows), N in {1, 4, 64, 512}.  HIP events around a window of --reps calls of each (the batch's guesses are reset by a
device-to-device copy, which the sequential loop's host-to-device copy per call corresponds to), a synchronisation after;
3 warm-up rounds, then 5 timed windows with the two versions alternating; per-call medians and the spread (max - min) of the
five, for every --max-nodes given (2048 fits these searches; 8192 is the ABI's default and shows what the larger grid costs).  Prints one JSON line per N and a verdict for
N = 64: the batch has to win by more than max(10 %, the spread).  Results are compared first: poses, counts and minima equal.

  python tools/search_batch_probe.py [--max-nodes 2048 8192] [--threshold 2.0] [--reps 0] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-nodes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--reps", type=int, default=0, help="calls per timed window; 0 = enough for about 512 searches")
    ap.add_argument("--threshold", type=float, default=2.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 4, 64, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import _capi, host, synth

    assert torch.cuda.is_available(), "the probe measures on a GPU"
    dev = torch.device("cuda:0")
    prob = synth.make_batch_problem(8, 64, 34)
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    mapp, clu = R.indoor_map_params(), R.indoor_cluster_params()
    subs = R.Maps(ctx, len(prob["submaps"]), mapp, mapp.size_x * mapp.size_y, with_grid=True)
    for j, sm in enumerate(prob["submaps"]):
        kf = torch.from_numpy(np.stack(sm["kf_scans"])).to(dev)
        tmp = R.Maps(ctx, kf.shape[0], mapp, 512, with_grid=False)
        R.ndt_build_batch(ctx, kf, clu, tmp)
        subs.merge(j, tmp, 0, synth.pose3_to_pose4(sm["kf_rel"]))
        tmp.close()
    B = len(prob["scans"])
    scans = R.Maps(ctx, B, mapp, 512, with_grid=False)
    R.ndt_build_batch(ctx, torch.from_numpy(prob["scans"]).to(dev), clu, scans)
    ctx.synchronize()
    mp, bp = R.default_matcher_params(), host.bnb_params(cost_threshold=args.threshold)
    start = synth.pose3_to_pose4(prob["truth"] + np.array([0.9, -0.7, 0.1]))
    fo = np.ascontiguousarray(prob["submap_of"], dtype=np.int32)
    st = torch.cuda.current_stream()
    lines = []
    for n, max_nodes in [(min(n, B), m) for n in args.sizes for m in args.max_nodes]:
        reps = args.reps if args.reps > 0 else max(1, 512 // n)
        fidx = torch.from_numpy(fo[:n]).to(dev)
        t0 = torch.from_numpy(np.ascontiguousarray(start[:n])).to(dev)
        t = t0.clone()
        res = torch.zeros((n, 16), dtype=torch.uint8, device=dev)

        def sequential():
            for _ in range(reps):
                out = [host.search_global(ctx, subs, int(fo[p]), scans, p, mp, bp, start[p]) for p in range(n)]
            return out

        def batch():
            for _ in range(reps):
                t.copy_(t0)
                host.search_global_batch_dev(ctx, subs, fidx, scans, 0, n, mp, bp, t, res, max_nodes=max_nodes)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            out = fn()
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps, out

        for _ in range(3):
            _, single = timed(sequential)
            timed(batch)
        r = res.cpu().numpy().view(_capi.BNB_RESULT_DTYPE).reshape(n)
        poses = t.cpu().numpy()
        same = bool((r["status"] == 0).all() and all(r["n_evals"][p] == single[p][2] and np.array_equal(poses[p], single[p][1]) and
                                                     r["min_cost"][p] == single[p][0] for p in range(n)))
        t_seq, t_bat = [], []
        for _ in range(5):
            t_seq.append(timed(sequential)[0])
            t_bat.append(timed(batch)[0])
        line = {"n_pairs": n, "threshold": args.threshold, "max_nodes": max_nodes, "calls_per_window": reps, "same_results": same,
                "evals_per_pair_mean": float(r["n_evals"].mean()), "found_a_minimum": int((r["min_cost"] < 100000.0).sum()),
                "sequential_ms": {"median": float(np.median(t_seq)), "spread": float(max(t_seq) - min(t_seq)), "runs": t_seq},
                "batch_ms": {"median": float(np.median(t_bat)), "spread": float(max(t_bat) - min(t_bat)), "runs": t_bat}}
        line["speedup"] = line["sequential_ms"]["median"] / line["batch_ms"]["median"]
        if n == 64:
            gain = 1.0 - line["batch_ms"]["median"] / line["sequential_ms"]["median"]
            bar = max(0.10, max(line["sequential_ms"]["spread"], line["batch_ms"]["spread"]) / line["sequential_ms"]["median"])
            line["requirement_at_64"] = {"gain": gain, "bar": bar, "met": bool(gain > bar)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0 if all(line["same_results"] for line in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
