"""Scan Context: the query entry (a scan outside the database, chunked candidate search) against the existing detect entry on
the database extended by the queries -- the composition tests/test_gpu_sc_query.py holds bit-equal.

  query     randt_sc_query_batch_dev   n_queries scans against n_db nodes
  baseline  randt_sc_detect_batch_dev  the same n_db nodes with the queries appended as nodes n_db .. n_db + n_queries - 1,
                                       num_exclude_recent = 1 (query j also sees the j queries before it: <= 15 of >= 1024 entries)

Shapes: n_db in {1024, 16384, 65536} x n_queries in {1, 16} at host.sc_params() defaults (20 rings, 45 sectors, 10 candidates).
Figures are HIP-event times per call over a window of calls that rotate over two distinct databases, enqueued behind a few
milliseconds of unrelated device work so that the window measures the device and not the host's enqueue rate.  Every figure is
the median of --reps windows with its spread (max - min) / median; the two sides are sampled alternately; everything is run
twice (run_a, run_b).  Both sides' answers for query 0 are compared bit for bit at every shape before anything is timed.

  python tools/sc_query_probe.py [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_DB = (1024, 16384, 65536)
N_QUERIES = (1, 16)
N_SETS = 2


def stats(samples):
    s = sorted(samples)
    med = s[len(s) // 2]
    return {"median_us": round(med, 3), "min_us": round(s[0], 3), "max_us": round(s[-1], 3), "spread": round((s[-1] - s[0]) / med, 4), "samples": len(s)}


def verdict(query, base):
    gain = 1.0 - query["median_us"] / base["median_us"]
    need = max(0.10, query["spread"], base["spread"])
    return {"gain": round(gain, 4), "needed": round(need, 4), "speedup": round(base["median_us"] / query["median_us"], 3),
            "faster_beyond_spread": bool(gain > need), "slower_beyond_spread": bool(-gain > max(query["spread"], base["spread"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=32, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    import torch

    import randt_slam_amd as R
    from randt_slam_amd import host

    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    ctx = R.Context(0, torch.cuda.current_stream().cuda_stream)
    sp_q = host.sc_params()
    sp_d = host.sc_params(num_exclude_recent=1)
    S, Rn, K = sp_q.num_sector, sp_q.num_ring, sp_q.num_candidates
    n_places = 512

    def database(n, seed):
        """n + 16 nodes on the device: sector rolls of n_places sparse integer places with a few perturbed bins (distinct keys,
        some exact duplicates), a random walk of positions; the last 16 nodes are the queries."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        places = torch.randint(1, 9, (n_places, S, Rn), generator=g, device=dev).to(torch.float64) * (torch.rand((n_places, S, Rn), generator=g, device=dev) < 0.3)
        which = torch.randint(0, n_places, (n + 16,), generator=g, device=dev)
        desc = places[which]
        shift = torch.randint(0, S, (n + 16,), generator=g, device=dev)
        idx = (torch.arange(S, device=dev)[None, :] - shift[:, None]) % S
        desc = torch.gather(desc, 1, idx[:, :, None].expand(-1, -1, Rn)).contiguous()
        bump = torch.randint(0, S * Rn, (n + 16, 8), generator=g, device=dev)
        desc.view(n + 16, -1).scatter_add_(1, bump, torch.ones_like(bump, dtype=torch.float64))
        rk = (desc.sum(1) / S).contiguous()                              # (integer bins: every order of the sum is exact)
        pos = torch.cumsum(0.4 * torch.randn((n + 16, 2), generator=g, device=dev, dtype=torch.float64), 0).contiguous()
        dist = torch.cumsum(0.3 + 0.4 * torch.rand((n + 16,), generator=g, device=dev, dtype=torch.float64), 0).contiguous()
        return desc, rk, pos, dist

    blocker = torch.randn((8192, 8192), dtype=torch.float32, device=dev)

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            torch.mm(blocker, blocker)                                   # the host gets ahead of the device while this runs
        e0.record()
        for i in range(launches):
            fn(i % N_SETS)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    result = {"params": {"num_ring": Rn, "num_sector": S, "num_candidates": K}, "reps": args.reps, "launches_per_window": args.launches, "shapes": {}}
    for n_db in N_DB:
        sets = [database(n_db, 1000 + n_db + k) for k in range(N_SETS)]
        for nq in N_QUERIES:
            out_q = (torch.zeros(nq, dtype=torch.int32, device=dev), torch.zeros(nq, dtype=torch.float32, device=dev), torch.zeros(nq, dtype=torch.float64, device=dev),
                     torch.zeros((nq, K), dtype=torch.int32, device=dev), torch.zeros((nq, K), dtype=torch.float32, device=dev),
                     torch.zeros((nq, K), dtype=torch.float64, device=dev))
            out_d = (torch.zeros(nq, dtype=torch.int32, device=dev), torch.zeros(nq, dtype=torch.float32, device=dev), torch.zeros(nq, dtype=torch.float64, device=dev))
            ids = torch.arange(n_db, n_db + nq, dtype=torch.int32, device=dev)

            def run_query(k):
                desc, rk, pos, dist = sets[k]
                host.sc_query_batch(ctx, sp_q, desc[:n_db], rk[:n_db], pos[:n_db], dist[:n_db], desc[n_db:n_db + nq], rk[n_db:n_db + nq], pos[n_db:n_db + nq],
                                    dist[n_db:n_db + nq], *out_q)

            def run_detect(k):
                desc, rk, pos, dist = sets[k]
                host.sc_detect_batch(ctx, sp_d, desc[:n_db + nq], rk[:n_db + nq], pos[:n_db + nq], dist[:n_db + nq], ids, *out_d)

            for k in range(N_SETS):                                      # query 0 searches exactly the n_db nodes on both sides
                run_query(k)
                run_detect(k)
                ctx.synchronize()
                same = all(torch.equal(a[:1].view(torch.int32) if a.dtype != torch.float64 else a[:1].view(torch.int64),
                                       b[:1].view(torch.int32) if b.dtype != torch.float64 else b[:1].view(torch.int64)) for a, b in zip(out_q[:3], out_d))
                assert same, "query and detect entries differ at n_db %d, n_queries %d" % (n_db, nq)
            for _ in range(2):                                           # warm-up of both sides at this shape
                window(run_detect, args.launches)
                window(run_query, args.launches)
            entry = {}
            for run in ("run_a", "run_b"):
                q_s, d_s = [], []
                for _ in range(args.reps):
                    q_s.append(window(run_query, args.launches))
                    d_s.append(window(run_detect, args.launches))
                entry[run] = {"query": stats(q_s), "baseline_detect": stats(d_s)}
                entry[run]["verdict"] = verdict(entry[run]["query"], entry[run]["baseline_detect"])
            entry["n_hits"] = int((out_q[0] >= 0).sum())
            result["shapes"]["n_db_%d_n_queries_%d" % (n_db, nq)] = entry
            print("n_db %6d  n_queries %2d   query %9.1f us   detect %9.1f us   (run_a medians)" %
                  (n_db, nq, entry["run_a"]["query"]["median_us"], entry["run_a"]["baseline_detect"]["median_us"]), flush=True)
        del sets
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
