#!/usr/bin/env python3
"""bench.py -- NDT registrations/sec on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic input: BASELINE config 4's batch of 512 independent
registrations (8 submaps x 64 scans; 2000-point radar scans vs 100x100-slot 0.5 m submaps, indoor parameter set), each
registration = NDT build from the raw points + association against its submap + the full GNC / Levenberg-Marquardt
solve, all on the GPU through the C ABI of librandt_hip.so.  Inputs are resident in HBM before the timed region starts.

Timed region: an UNTIMED settle region of at least --min-seconds first (clocks, caches, allocator; it is clocked on the
side and reported as `sustained` = the rate the path holds when steps keep coming), then EXACTLY --steps steps between
barrier + synchronize on both sides -- the headline `value`.  The exact-K region is run --repeats times, each fully
bracketed; the median region is reported, all are listed.  A K-step region pays the pipeline's fill and drain (a step's
three launches last ~0.3 ms under load): with the driver's K = 20 the headline is a BURST figure, `sustained` the steady one.

Multi-GPU (launched by torch.distributed.run, one rank per GPU; "nccl" = RCCL over xGMI).  Independent registrations
shard with no data-path collective; the only collectives are the set-up broadcast of the submap tables and the result
gather.  Two regions are timed at N > 1 (the strong one only with --full or --scaling strong):
  * weak   (the headline `value`): every rank processes its own 512-registration batch per step;
  * strong (`strong_scaling`): BASELINE config 4 as written -- ONE batch of 512 (seeds 1000..1511) split contiguously,
    rank r runs [r*512/N, (r+1)*512/N), results all-gathered and checked bit-identical to the unsharded batch.

Roofline: this path is not HBM-bound (counter traffic is ~10x below the dense-table byte model) but VALU-issue bound
(fp64 vector instructions, no MFMA: J^T J is a reduction, not a GEMM).  `roofline` therefore prices the dominant kernel
against the VALU issue rate: counted instructions per launch (rocprofv3 SQ counters, profiles/*_sq_summary.csv) x
measured issue cycles per instruction class (tools/valu_rate_probe.hip) / the launch duration measured here with HIP
events, over 1024 SIMDs x 2.4 GHz.  The SURVEY byte model and the counter traffic are kept as labelled secondaries.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) does only what the headline needs: set-up, warm-up (W steps per
stream, the settle region, then up to 8 untimed K-step regions within about a second; none of it reported), ONE region of
exactly K timed steps, and the line.  --full adds
everything else: `sustained`, the --repeats median (9 regions), the strong / pipelined multi-GPU regions, `hbm_achieved`,
the roofline sections, the CPU baselines and the side measurements of the other BASELINE configs.

--dump-outputs DIR writes what the timed path returned in its last step, as float64 .npy files: `pose.npy` (B x 4, the
solved poses as cos, sin, x, y) and `result_<field>.npy` (B, one per field of the 64-byte result record).  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.

Prints ONE JSON line on rank 0.
"""
import argparse
import csv
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_SUBMAPS, SCANS_PER_SUBMAP, N_KEYFRAMES = 8, 64, 34
N_POINTS, N_SLOTS = 2000, 100 * 100
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6    # vector fp64 (half the 157.3 TF fp32 vector rate)
N_SIMDS, CLOCK_GHZ = 1024, 2.4          # 256 CUs x 4 SIMDs, max clock (MI355X_MICROARCH.md chip table)
VALU_PEAK = N_SIMDS * CLOCK_GHZ         # G SIMD-cycles/s of VALU issue
SAT_COPIES = 16                         # chip-filling launch of the roofline section: 16 copies of the batch = 8192 registrations =
                                        # exactly two rounds of the 4096 resident wavefronts (4 per SIMD) of the one-wavefront solve kernel
HOT_KERNELS = ("k_ndt_build<true,true>", "k_associate<false,64,true,false>", "k_solve<3,1,64,true,4,false>")


ALL_ROWS = []      # every row of the committed counter summary (empty when the counters are refused as stale)
WINDOW_ROW = {}    # counter row of k_solve_window (the fixed-lag solve of config 3) from the committed summary
FILTER_ROWS = {}   # counter rows of k_filter_rows / k_filter_emit from the committed summary (load_counters)


def effective_cpus():
    """CPUs this process may really use: the affinity mask capped by the cgroup CPU quota (the GPU boxes of this pool show
    256 logical CPUs behind a 16-CPU quota: 128 OpenMP threads there are 16 cores' worth of time slices)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(p)
    except Exception:  # noqa: BLE001
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except Exception:  # noqa: BLE001
            pass
    eff = n if quota is None else max(1, min(n, int(quota)))
    return eff, n, quota


def algorithmic_bytes(n_points, n_slots, m_cells, k):
    """bytes one registration must move (points in, dense submap table + index grid,
    scan cells out + back in, correspondences, pose/stat out)."""
    return n_points * 16 + n_slots * 48 + n_slots * 4 + m_cells * 48 * 2 + m_cells * k * 4 + 64


def load_counters():
    """Latest committed profiles/r*_sq_summary.csv (tools/pmc_summary.py): per-launch SQ / TCC counters of the three hot
    kernels at the 512-registration launch.  Returns ({kernel: row dict}, file name, stale reason or None): counters stamped
    with another fingerprint of the hot kernels' sources (tools/csrc_hash.py) than the code being benchmarked are REFUSED."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from csrc_hash import csrc_hash

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sq_summary.csv")))
    if not files:
        return {}, None, "no committed counter summary"
    rows = {}
    FILTER_ROWS.clear()
    WINDOW_ROW.clear()
    del ALL_ROWS[:]
    want_wgs = {"k_ndt_build<true,true>": 512, "k_associate<false,64,true,false>": 128, "k_solve<3,1,64,true,4,false>": 128}   # workgroups of a 512-registration launch (the association walks four pairs per workgroup)
    stamp = None
    for r in csv.DictReader(open(files[-1])):
        stamp = r.get("csrc_hash", stamp)
        ALL_ROWS.append({k: (float(v) if v not in ("", None) and k not in ("kernel", "csrc_hash") else v) for k, v in r.items()})
        if r["kernel"].startswith("k_filter_") and r["kernel"] not in FILTER_ROWS:     # the config-5 polar filter (16 scans per launch)
            FILTER_ROWS[r["kernel"]] = {k: (float(v) if v not in ("", None) and k not in ("kernel", "csrc_hash") else v) for k, v in r.items()}
        if r["kernel"].startswith("k_solve_window<") and not WINDOW_ROW:
            WINDOW_ROW.update({k: (float(v) if v not in ("", None) and k not in ("kernel", "csrc_hash") else v) for k, v in r.items()})
        if r["kernel"] in HOT_KERNELS and r["kernel"] not in rows and int(r["grid_size"]) == want_wgs[r["kernel"]] * int(r["workgroup_size"]):
            rows[r["kernel"]] = {k: (float(v) if v not in ("", None) and k not in ("kernel", "csrc_hash") else v) for k, v in r.items()}
    rel = os.path.relpath(files[-1], ROOT)
    now = csrc_hash()
    if stamp != now:
        del ALL_ROWS[:]
        return {}, rel, "counters in %s were taken from other kernel code (stamp %s, current sources %s): re-run tools/collect_profiles.sh" % (rel, stamp, now)
    return rows, rel, None


def row_bytes(r):
    """HBM bytes of one dispatch from its TCC counters: FETCH_SIZE KB x 2 (the gfx950 correction of MI355X_MICROARCH.md) + WRITE_SIZE KB."""
    return (2.0 * r.get("FETCH_SIZE", 0.0) + r.get("WRITE_SIZE", 0.0)) * 1024.0


def find_row(prefix, grid=None, most_dispatched_below=None):
    """A row of the committed counter summary: kernel name starting with `prefix`, at `grid` threads, or -- among launches of at
    most `most_dispatched_below` threads -- the one the collection run dispatched most often (the per-scan launches of the
    odometry drive that is part of every collection run)."""
    best = None
    for r in ALL_ROWS:
        if not r["kernel"].startswith(prefix):
            continue
        if grid is None and most_dispatched_below is None:
            return r                       # any launch size: the first (heaviest) row of that kernel
        if grid is not None and int(r["grid_size"]) == grid:
            return r
        if most_dispatched_below is not None and int(r["grid_size"]) <= most_dispatched_below and (best is None or r["dispatches"] > best["dispatches"]):
            best = r
    return best


def hbm_achieved(counters, ms_per_step, sustained_ms_per_step, counters_file, counters_stale):
    """north_star's "achieved HBM-bandwidth fraction" of the headline path, from counters: FETCH_SIZE x 2 + WRITE_SIZE of the three
    launches of a 512-registration step / the step time / 8 TB/s.  SURVEY 8(d) expected 1 .. 10 %: the path is bound by vector-ALU
    issue slots and the latency of its dependent chains (roofline), not by bytes."""
    if counters_stale or not all(n in counters for n in HOT_KERNELS):
        return {"frac": None, "counters_refused": counters_stale or "no counter rows for the three kernels"}
    by = {n: row_bytes(counters[n]) for n in HOT_KERNELS}
    tot = sum(by.values())
    out = {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "bytes_per_step": int(tot), "bytes_by_kernel": {n: int(v) for n, v in by.items()},
           "bytes_per_registration": tot / 512.0, "achieved": tot / (ms_per_step * 1e-3) / 1e9, "frac": tot / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "counters": counters_file,
           "note": "PMC bytes of the three launches of one 512-registration step (FETCH_SIZE x 2 + WRITE_SIZE, %s) / ms_per_step of "
                   "the headline region; `sustained`: the same over the settle region's step" % counters_file}
    if sustained_ms_per_step:
        out["sustained"] = {"achieved": tot / (sustained_ms_per_step * 1e-3) / 1e9, "frac": tot / (sustained_ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS}
    return out


DUMP_BYTES_MAX = 64 << 20


def write_outputs(dirname, pose, records):
    """--dump-outputs: the poses (B x 4) and result records (B) of the timed path's last step, as float64 .npy files.  Above
    DUMP_BYTES_MAX in all (only at a large --batch-scale) a fixed seeded sample of the rows is written, its indices in rows.npy."""
    fields = [f for f in records.dtype.names if f != "reserved"]
    n_max = DUMP_BYTES_MAX // (8 * (pose.shape[1] + len(fields) + 1))
    os.makedirs(dirname, exist_ok=True)
    rows = slice(None)
    if len(pose) > n_max:
        rows = np.sort(np.random.default_rng(0).choice(len(pose), n_max, replace=False))
        np.save(os.path.join(dirname, "rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(dirname, "pose.npy"), np.asarray(pose[rows], dtype=np.float64))
    for f in fields:
        np.save(os.path.join(dirname, "result_%s.npy" % f), records[f][rows].astype(np.float64))


class GroupBatch:
    """BASELINE config 4 as written -- ONE batch split over the GPUs of the node -- through the C ABI's multi-GPU group
    (randt_group_scan_register_batch_dev): every rank holds the full input arrays, runs its contiguous shard (NDT build ->
    associate -> solve) and the (pose, record) rows are gathered in ONE exchange per step (packed 96-byte rows, one
    ncclAllGather) on the group's stream.  Several groups (one communicator + stream each) keep several batches in flight:
    step j goes to group j % len(groups) -- what a loop-closure burst on the node would run."""

    def __init__(self, R, torch, groups, submaps_gs, mapp, clu, mp, points, fixed_idx, guess4, scan_cap=512, gather=True):
        self.groups, self.submaps_gs, self.clu, self.mp, self.gather = groups, submaps_gs, clu, mp, gather
        self.points, self.fixed_idx, self.guess4 = points, fixed_idx, guess4
        self.B = int(points.shape[0])
        lo, hi = R.shard_range(self.B, groups[0].world, groups[0].first_rank)
        self.lo, self.hi = lo, hi
        self.poses = [guess4.clone() for _ in groups]
        self.results = [torch.zeros((self.B, 64), dtype=torch.uint8, device=points.device) for _ in groups]
        self.ws = [R.Maps(g.ctxs[0], max(1, hi - lo), mapp, scan_cap, with_grid=False) for g in groups]

    def step(self, j, stream, pose, events=None, only=None):
        g = j % len(self.groups)
        if events is not None:
            events[0].record(stream)
            events[1].record(stream)
            events[2].record(stream)
        self.groups[g].scan_register_batch([self.points], self.clu, [self.submaps_gs[g]], [self.fixed_idx], [self.ws[g]], self.mp, [pose],
                                           [self.results[g]], gather=self.gather)
        if events is not None:
            events[3].record(stream)


class Batch:
    """One batch of registrations resident in HBM + the per-stream working sets of the three launches."""

    def __init__(self, R, torch, ctxs, submaps_v, mapp, clu, mp, points, fixed_idx, guess4, scan_cap=512):
        self.R, self.torch, self.ctxs, self.submaps_v, self.clu, self.mp = R, torch, ctxs, submaps_v, clu, mp
        self.points, self.fixed_idx, self.guess4 = points, fixed_idx, guess4
        self.B = int(points.shape[0])
        n, k, dev = len(ctxs), mp.n_neighbours, points.device
        self.poses = [guess4.clone() for _ in range(n)]
        self.results = [torch.zeros((self.B, 64), dtype=torch.uint8, device=dev) for _ in range(n)]
        self.corrs = [torch.full((self.B, scan_cap, k), -1, dtype=torch.int32, device=dev) for _ in range(n)]
        self.scan_maps = [R.Maps(ctxs[i], self.B, mapp, scan_cap, with_grid=False) for i in range(n)]
        self.points_rotation, self._turn = None, 0   # distinct_inputs: a list of point batches at different addresses, one per step in turn

    def step(self, j, stream, pose, events=None, only=None):
        """Enqueue build -> associate -> solve of the whole batch on stream slot j (asynchronous)."""
        R, cx = self.R, self.ctxs[j]
        if self.points_rotation is not None:
            self.points = self.points_rotation[self._turn % len(self.points_rotation)]
            self._turn += 1
        if events is not None:
            events[0].record(stream)
        if only in (None, "build", "no-associate"):
            R.ndt_build_batch(cx, self.points, self.clu, self.scan_maps[j])
        if events is not None:
            events[1].record(stream)
        if only in (None, "associate", "no-build"):
            R.associate_batch(cx, self.submaps_v[j], self.fixed_idx, self.scan_maps[j], 0, self.B, pose, self.mp, self.corrs[j])
        if events is not None:
            events[2].record(stream)
        if only in (None, "solve", "no-build", "no-associate"):
            R.solve_batch(cx, self.submaps_v[j], self.fixed_idx, self.scan_maps[j], 0, self.B, self.corrs[j], self.mp, pose, self.results[j])
        if events is not None:
            events[3].record(stream)


# Steps whose three launches are bracketed by HIP events (stage residency while batches overlap); the others enqueue the
# kernels only.  An event record is a barrier + signal packet on its queue: four of them per step cost 7 % of the
# throughput (61.5 -> 57.3 us per step without any), and a spacing that shares a factor with the stream count piles them
# onto the same streams (every 8th: 63.9 us) -- so every 67th step (prime) is instrumented; the roofline's launch
# durations come from the dedicated single-stream sections, where every launch is bracketed.
EVENT_EVERY = 67


def timed_region(torch, dist, world, dev, batch, streams, n_steps, only=None):
    """EXACTLY n_steps steps between barrier + synchronize on both sides; MAX over ranks.  The initial guess is an input
    and the solve updates it in place (Sophus::SE2d& trans): every step gets its own copy, resident beforehand; the
    last step's is returned."""
    n_streams = len(streams)
    step_pose = [batch.guess4.clone() for _ in range(n_steps)]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] if s % EVENT_EVERY == EVENT_EVERY // 2 or n_steps <= EVENT_EVERY and s == n_steps // 2
          else None for s in range(n_steps)]
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(n_steps):
        j = s % n_streams
        batch.step(j, streams[j], step_pose[s], ev[s], only)
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    stage_ms = np.array([[ev[s][i].elapsed_time(ev[s][i + 1]) for i in range(3)] for s in range(n_steps) if ev[s] is not None] or [[0.0] * 3]).mean(axis=0)
    return elapsed, t_enq, stage_ms, step_pose[-1]


def warm_up(torch, batch, streams, n):
    for i in range(n):
        j = i % len(streams)
        with torch.cuda.stream(streams[j]):
            batch.poses[j].copy_(batch.guess4)
        batch.step(j, streams[j], batch.poses[j])
    torch.cuda.synchronize()


_HUNG_THREADS = []   # watchdog victims (a collective that never returned): the process leaves through os._exit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000, help="steps of the timed region (exactly this many)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.3, help="length of the untimed settle region in front of the timed one (clocked on the side: `sustained`)")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the exact --steps region is run this many times (median reported, all listed); default 9 with --full, else 1")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: sustained rate, repeats, strong scaling, roofline, CPU baselines and "
                         "the side measurements of the other configs (their options below only act with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the poses and result records of the timed path's last step to DIR/*.npy (float64)")
    ap.add_argument("--scaling", choices=["weak", "strong", "both"], default="both",
                    help="multi-GPU regions to time (the headline value is the weak one unless only strong is asked for)")
    ap.add_argument("--batch-scale", type=int, default=1,
                    help="diagnostic: registrations per step = 512 x this (the headline workload is 1)")
    ap.add_argument("--only", choices=["build", "associate", "solve", "no-build", "no-associate"], default=None,
                    help="diagnostic: time ONE stage alone at saturation (the printed value is then not the headline metric)")
    ap.add_argument("--streams", type=int, default=16, help="in-flight batches: step i runs on HIP stream i %% streams "
                    "(GPU_MAX_HW_QUEUES is raised to match unless already set: HIP maps streams onto 4 hardware queues by default)")
    ap.add_argument("--solve-mode", choices=["default", "auto", "throughput"], default="default",
                    help="pair-solve geometry of the timed region's contexts: throughput = one wavefront per registration, auto = the "
                         "library's choice per launch (splits a lone small batch); default = throughput when several streams keep batches in flight")
    ap.add_argument("--odometry-scans", type=int, default=1000, help="BASELINE config 3 side measurement (0 = skip)")
    ap.add_argument("--distinct-inputs", type=int, default=20,
                    help="side measurement: the headline region again over this many copies of the point batch at distinct addresses (> 256 MB; 0 / 1 = skip)")
    ap.add_argument("--no-auto-region", action="store_true", help="skip the headline region with the contexts in RANDT_SOLVE_AUTO")
    ap.add_argument("--replica-steps", type=int, default=150,
                    help="side measurement: R = 64 / 256 replicas of config 3's loop in lock-step, this many steps each (0 = skip)")
    ap.add_argument("--cpp-drive-scans", type=int, default=300,
                    help="side measurement: the drop-in path driven from C++ with host buffers and Maps by value (tests/cpp/local_fuser_drive.cpp; 0 = skip)")
    ap.add_argument("--polar-scans", type=int, default=16, help="BASELINE config 5 side measurement: polar filter (0 = skip)")
    ap.add_argument("--slam-scans", type=int, default=300,
                    help="side measurement: whole SLAM call pattern (odometry + loop closure + pose graph) on a two-lap drive (0 = skip)")
    ap.add_argument("--polar-odometry-scans", type=int, default=60,
                    help="BASELINE config 5 side measurement: full local-fuser loop on raw polar scans (0 = skip)")
    ap.add_argument("--event-every", type=int, default=EVENT_EVERY, help="bracket the launches of every N-th timed step with HIP events (stage residency)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-group-path", action="store_true",
                    help="test hook: run the multi-GPU code path (randt_group over RCCL; strong regions with --full) with ONE rank on one GPU")
    ap.add_argument("--no-config2", action="store_true", help="skip the single-pair latency section (BASELINE config 2)")
    ap.add_argument("--no-roofline-sections", action="store_true", help="skip the single-stream / chip-filling-launch sections")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="wall-clock budget of each CPU baseline leg")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 9 if args.full else 1

    globals()["EVENT_EVERY"] = max(1, args.event_every)
    # in-flight batches need their own hardware queues to overlap (must be set before the HIP runtime starts)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(max(4, min(32, args.streams))))
    import torch
    import torch.distributed as dist

    import randt_slam_amd as R
    from randt_slam_amd import shard, synth

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node %d bench.py --gpus %d ..." % (args.gpus, args.gpus))
    n_dev = torch.cuda.device_count()
    backend = os.environ.get("RANDT_BENCH_BACKEND", "nccl")
    # RANDT_RANKS_SHARE_GPU=1 (set by randt_slam_amd.shard.shared_gpu_rank_env, tests only): every rank sits on GPU 0 and RCCL is
    # told they are one-GPU nodes (NCCL_HOSTID), so the multi-rank RCCL path runs on a one-GPU box.  Never a scaling number:
    # the line carries `ranks_share_one_gpu`.
    share_gpu = os.environ.get("RANDT_RANKS_SHARE_GPU") == "1" and world > 1
    if local_rank >= n_dev and backend != "gloo" and not share_gpu:
        raise SystemExit("rank %d has no GPU (%d visible)" % (local_rank, n_dev))
    local_rank = local_rank % max(1, n_dev)   # only differs in the single-GPU gloo logic test and under RANDT_RANKS_SHARE_GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 or args.force_group_path:
        # "nccl" IS RCCL on ROCm.  RANDT_BENCH_BACKEND=gloo exists only to exercise the multi-rank control flow on a box
        # with fewer GPUs than ranks (tests); it is never used for reported numbers.
        if world == 1:   # --force-group-path: a one-rank process group, so that the unique-id broadcast / agreement code runs as written
            dist.init_process_group(backend="nccl", device_id=dev, init_method="tcp://127.0.0.1:%s" % os.environ.get("MASTER_PORT", "29561"),
                                    rank=0, world_size=1)
        elif backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)
    via_cpu = world > 1 and backend != "nccl"
    multi = world > 1 or args.force_group_path   # --force-group-path: the multi-GPU code (groups, strong regions, JSON keys) on ONE rank
    # the strong regions are the headline only under --scaling strong; with the default "both" they are a --full figure
    run_strong = multi and (args.scaling == "strong" or (args.full and args.scaling == "both"))

    # One randt context per HIP stream: consecutive steps (independent batches) alternate streams so
    # that the latency-bound tail of one batch's solve overlaps the next batch's build / association.
    n_streams = max(1, args.streams)
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream(device=dev) for _ in range(n_streams - 1)]
    ctxs = [R.Context(local_rank, st.cuda_stream) for st in streams]
    ctx = ctxs[0]
    throughput_mode = args.solve_mode == "throughput" or (args.solve_mode == "default" and n_streams > 1)
    if throughput_mode:
        # several batches in flight: the chip is full, one wavefront per registration (the library's AUTO default would give a
        # lone 512-registration batch eight wavefronts per registration -- right for the single_batch section below, which
        # switches it back, and wrong here: 4.6 M instead of 9.0 M registrations/s)
        for c in ctxs:
            c.set_solve_mode(R._capi.SOLVE_THROUGHPUT)
    mapp, clu = R.indoor_map_params(), R.indoor_cluster_params()
    mp = R.default_matcher_params()
    k = mp.n_neighbours
    scans_per_submap = SCANS_PER_SUBMAP * max(1, args.batch_scale)
    B = N_SUBMAPS * scans_per_submap

    # ---------------- set-up (untimed): synthetic world, scans, submaps ---------------------------
    # base problem = BASELINE config 4 (seeds 1000...): every rank generates it (deterministic); the submap tables are
    # BUILT on rank 0 only and broadcast (RCCL), like a deployment where one rank owns the submap epoch
    base = synth.make_batch_problem(N_SUBMAPS, scans_per_submap, N_KEYFRAMES)
    cb, nb, gb = R.Maps.storage_bytes(N_SUBMAPS, mapp, N_SLOTS)
    t_cells = torch.zeros(cb, dtype=torch.uint8, device=dev)       # torch-owned HBM so that RCCL can broadcast the tables
    t_counts = torch.zeros(N_SUBMAPS, dtype=torch.int32, device=dev)
    t_grid = torch.zeros(gb // 4, dtype=torch.int32, device=dev)
    submaps = R.Maps(ctx, N_SUBMAPS, mapp, N_SLOTS, storage=(t_cells, t_counts, t_grid))
    if rank == 0:
        for j, sm in enumerate(base["submaps"]):
            kf = torch.from_numpy(np.stack(sm["kf_scans"])).to(dev)
            tmp = R.Maps(ctx, kf.shape[0], mapp, 512, with_grid=False)
            R.ndt_build_batch(ctx, kf, clu, tmp)
            submaps.merge(j, tmp, 0, synth.pose3_to_pose4(sm["kf_rel"]))  # rolling-submap path (a9 + a18)
            tmp.close()
    ctx.synchronize()
    t_bcast = 0.0
    grp = submaps_g = None
    group_error = None
    extra_groups, extra_submaps = [], []

    def make_group(stream):
        """One multi-GPU group of the C ABI (csrc/group.hip: RCCL opened and driven by librandt_hip.so itself; torch.distributed only
        ships the 128-byte communicator id) on `stream`.  ncclCommInitRank is a collective: should it ever hang (a rank that could
        not open librccl, a bootstrap socket that does not connect) the bench must still produce its line -- the creation runs
        under a watchdog, a rank that gives up says so, and ALL ranks agree (all-reduce) whether the group exists."""
        import threading

        uid = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            uid.copy_(torch.from_numpy(R.group_unique_id()))
        dist.broadcast(uid, src=0)
        uid_host = uid.cpu().numpy()
        box = {}

        def _make():
            try:
                box["grp"] = R.Group(device=local_rank, rank=rank, world=world, unique_id=uid_host, stream=stream.cuda_stream)
            except Exception as e:  # noqa: BLE001 -- every rank must take the same path: agree below
                box["err"] = "%s" % e

        th = threading.Thread(target=_make, daemon=True)
        th.start()
        th.join(float(os.environ.get("RANDT_BENCH_GROUP_TIMEOUT", "120")))
        if th.is_alive():
            box["err"] = "no answer from randt_group_create_rank within the watchdog time"
            _HUNG_THREADS.append(th)
        g, sm, err = box.get("grp"), None, box.get("err")
        if g is not None and err is None:
            try:
                sm = R.Maps(g.ctxs[0], N_SUBMAPS, mapp, N_SLOTS, storage=(t_cells, t_counts, t_grid), clear=False)
            except Exception as e:  # noqa: BLE001
                g, err = None, "%s" % e
        else:
            g = None
        if err:
            sys.stderr.write("rank %d: randt_group unavailable (%s)\n" % (rank, err))
        ok = torch.tensor([1 if g is not None else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            return None, None, err or "another rank could not create its group member"
        return g, sm, None

    if multi:
        if not via_cpu:
            grp, submaps_g, group_error = make_group(streams[0])
            if grp is None:
                sys.stderr.write("rank %d: falling back to torch.distributed for the exchanges\n" % rank)
            elif run_strong:
                # further groups (own communicator, own stream): several split batches in flight for the pipelined strong region
                for j in range(1, max(1, min(int(os.environ.get("RANDT_BENCH_STRONG_GROUPS", "4")), n_streams))):
                    g2, sm2, e2 = make_group(streams[j])
                    if g2 is None:
                        break
                    extra_groups.append(g2)
                    extra_submaps.append(sm2)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        if via_cpu:
            for t in (t_cells, t_counts, t_grid):
                h = t.cpu()
                dist.broadcast(h, src=0)
                t.copy_(h)
        elif grp is None:
            shard.broadcast_submap_tables((t_cells, t_counts, t_grid), src=0)
        else:
            grp.broadcast_maps([submaps_g], root=0)                              # the only set-up collective (ncclBroadcast x 3)
            grp.synchronize()
        torch.cuda.synchronize()
        t_bcast = time.perf_counter() - t0
    submaps_v = [submaps] + [R.Maps(ctxs[i], N_SUBMAPS, mapp, N_SLOTS, storage=(t_cells, t_counts, t_grid), clear=False)
                             for i in range(1, n_streams)]

    def to_dev(prob, lo=0, hi=None):
        hi = len(prob["scans"]) if hi is None else hi
        return (torch.from_numpy(prob["scans"][lo:hi]).to(dev), torch.from_numpy(prob["submap_of"][lo:hi]).to(dev),
                torch.from_numpy(synth.pose3_to_pose4(prob["guess"][lo:hi])).to(dev))

    # weak region: rank r > 0 registers its OWN 512 scans (other seeds) against the same submaps
    if rank == 0 or args.scaling == "strong":
        weak_prob = base
    else:
        weak_prob = synth.make_batch_problem(N_SUBMAPS, scans_per_submap, N_KEYFRAMES, scan_seed0=1000 + 100000 * rank,
                                             guess_seed0=2000 + 100000 * rank)
    full = Batch(R, torch, ctxs, submaps_v, mapp, clu, mp, *to_dev(weak_prob))
    warm_up(torch, full, streams, args.warmup * n_streams)

    # ---------------- timed region (weak = the headline) --------------------------------------------
    # settle (untimed for the headline, clocked on the side), then EXACTLY args.steps steps, args.repeats times; `elapsed` is
    # already the maximum over ranks, so every rank takes the same decisions.  Without --full the settle region is warm-up
    # only and does not grow with --steps, so that a long timed region is not paid for twice.
    def settle(batch, use_streams=None):
        n, best = max(args.steps if args.full else 0, 16 * n_streams), None
        if args.min_seconds <= 0:
            return None
        for _ in range(6):
            r = timed_region(torch, dist, world, dev, batch, use_streams or streams, n, args.only)
            best = (n,) + r
            if r[0] >= args.min_seconds:
                break
            n = int(math.ceil(n * max(1.5, 1.25 * args.min_seconds / max(r[0], 1e-9))))
        return best

    def region(batch, use_streams=None):
        sus = settle(batch, use_streams)
        if not args.full and sus is not None:
            # the first K-step regions after the settle run slower (K = 20: 2.0 ms, then down to 1.7 ms by the 8th), which the
            # --full median of 9 never reports: up to 8 identical regions run untimed first, while they fit in about a second
            est, spent = args.steps * sus[1] / sus[0], 0.0
            for _ in range(8):
                if spent + est > 1.0:
                    break
                spent += timed_region(torch, dist, world, dev, batch, use_streams or streams, args.steps, args.only)[0]
        runs =[timed_region(torch, dist, world, dev, batch, use_streams or streams, args.steps, args.only) for _ in range(max(1, args.repeats))]
        order = sorted(range(len(runs)), key=lambda i: runs[i][0])
        r = runs[order[len(order) // 2]]
        info = {"repeats": len(runs), "region_ms": [x[0] * 1e3 for x in runs]}
        if sus is not None and args.full:
            info["sustained"] = {"steps": sus[0], "timed_region_s": sus[1], "ms_per_step": sus[1] / sus[0] * 1e3,
                                 "value": batch.B * sus[0] * (world if batch is full else 1) / sus[1], "unit": "registrations/s",
                                 "stage_ms": [float(v) for v in sus[3]],
                                 "note": "the settle region in front of the timed one: %d steps back to back on %d streams, same bracketing; "
                                         "the steady rate (what rounds 1-3 reported as the headline)" % (sus[0], len(use_streams or streams))}
        return (args.steps,) + r + (info,)

    out = {}
    if args.scaling != "strong" or world == 1:
        n_steps, elapsed, t_enqueued, stage_ms, last_pose, rinfo = region(full)
        value = B * n_steps * world / elapsed
        scaling = "weak"
        if args.dump_outputs:   # copied now: the --full sections below reuse the batch's buffers
            dump = (last_pose.cpu(), full.results[(n_steps - 1) % n_streams].cpu())
    strong = None
    if run_strong:
        lo, hi = shard.shard_range(B, world, rank)
        extra = {}
        if grp is not None:
            # through the C ABI: shard + kernels + ONE RCCL exchange of the packed (pose, record) rows inside every step
            part = GroupBatch(R, torch, [grp], [submaps_g], mapp, clu, mp, *to_dev(base))
            warm_up(torch, part, streams[:1], 4)
            s_steps, s_elapsed, s_enq, s_stage, s_last_pose, s_info = region(part, streams[:1])
            all_pose, all_res, t_gather = s_last_pose, part.results[0], None
            how = "randt_group_scan_register_batch_dev (C ABI, one ncclAllGather of packed 96-byte rows inside every step, one stream)"
            # the same region without the exchange: what the kernels alone cost per step
            nog = GroupBatch(R, torch, [grp], [submaps_g], mapp, clu, mp, *to_dev(base), gather=False)
            warm_up(torch, nog, streams[:1], 4)
            k_steps, k_elapsed = region(nog, streams[:1])[:2]
            extra["kernel_us_per_step"] = k_elapsed / k_steps * 1e3 * 1e3
            extra["gather_us_per_step"] = (s_elapsed / s_steps - k_elapsed / k_steps) * 1e6
            # several split batches in flight (one group = communicator + stream each)
            groups, gsubs = [grp] + extra_groups, [submaps_g] + extra_submaps
            if len(groups) > 1:
                pipe = GroupBatch(R, torch, groups, gsubs, mapp, clu, mp, *to_dev(base))
                warm_up(torch, pipe, streams[:len(groups)], 2 * len(groups))
                p_steps, p_elapsed, _, _, _, p_info = region(pipe, streams[:len(groups)])
                extra["pipelined"] = {"groups_in_flight": len(groups), "steps": p_steps, "ms_per_step": p_elapsed / p_steps * 1e3,
                                      "value": B * p_steps / p_elapsed, "unit": "registrations/s", "region_ms": p_info["region_ms"],
                                      "sustained": p_info.get("sustained"),
                                      "note": "the same split batch, %d of them in flight (one RCCL communicator + stream each): what a "
                                              "loop-closure burst on the node runs" % len(groups)}
        else:
            part = Batch(R, torch, ctxs, submaps_v, mapp, clu, mp, *to_dev(base, lo, hi))
            warm_up(torch, part, streams, 2 * n_streams)
            s_steps, s_elapsed, s_enq, s_stage, s_last_pose, s_info = region(part)
            # result gather (all-gather of 32-B poses + 64-B records) and the bit-identity check against the unsharded batch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp, lr = (s_last_pose.cpu(), part.results[0].cpu()) if via_cpu else (s_last_pose, part.results[0])
            all_pose = shard.gather_results(lp)
            all_res = shard.gather_results(lr)
            torch.cuda.synchronize()
            t_gather = time.perf_counter() - t0
            how = "per-rank randt_scan_register_batch_dev, gather through torch.distributed (gloo control-flow test only)"
        strong = {"value": B * s_steps / s_elapsed, "unit": "registrations/s", "scaling": "strong", "steps": s_steps,
                  "ms_per_step": s_elapsed / s_steps * 1e3, "registrations_per_gpu_per_step": hi - lo,
                  "workload": "ONE 512-registration batch (seeds 1000..1511) split contiguously over %d GPUs" % world,
                  "entry": how,
                  "stage_ms": {"ndt_build": float(s_stage[0]), "associate": float(s_stage[1]), "solve": float(s_stage[2])},
                  "result_gather_ms": None if t_gather is None else t_gather * 1e3, "submap_broadcast_ms": t_bcast * 1e3,
                  "submap_broadcast_bytes": int(cb + nb + gb), "repeats": s_info["repeats"], "region_ms": s_info["region_ms"],
                  "sustained": s_info.get("sustained"),
                  "expected_ceiling": "a lone 512-registration batch lasts ~159 us on one GPU (build 31 + associate 24 + split solve 104) and its "
                                      "64-registration share of an 8-GPU split ~133 us: both are the LATENCY of the longest registration's chain of "
                                      "passes, which sharding does not shorten -- at most 159 / 133 = 1.2x from 1 to 8 GPUs before the gather is paid; "
                                      "the strong curve of ONE batch is flat by construction (see `pipelined` for several batches in flight, and the "
                                      "weak region for throughput)"}
        strong.update(extra)
        if rank == 0:
            ref = Batch(R, torch, ctxs[:1], submaps_v[:1], mapp, clu, mp, *to_dev(base))
            rp = ref.guess4.clone()
            ref.step(0, streams[0], rp)
            torch.cuda.synchronize()
            strong["poses_bit_identical_to_unsharded"] = bool(torch.equal(all_pose.cpu(), rp.cpu()) and
                                                              torch.equal(all_res.cpu(), ref.results[0].cpu()))
        if args.scaling == "strong":
            n_steps, elapsed, t_enqueued, stage_ms, last_pose, value, scaling, rinfo = s_steps, s_elapsed, s_enq, s_stage, s_last_pose, strong["value"], "strong", s_info
            if args.dump_outputs:
                dump = (all_pose.cpu(), all_res.cpu())

    if rank == 0:
        res = full.results[0].cpu().numpy().view(R.RESULT_DTYPE).reshape(-1)
        m_mean = float(full.scan_maps[0].counts().mean())
        n_res_mean = float(res["n_residuals"].mean())
        out = {
            "metric": "ndt_registrations_per_sec" if args.only is None and args.batch_scale == 1 else "DIAGNOSTIC_only=%s_batch_scale=%d" % (args.only, args.batch_scale),
            "value": value, "unit": "registrations/s",
            "n_gpus": world, "steps": n_steps, "steps_requested": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / n_steps * 1e3, "timed_region_s": elapsed, "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {
                "workload": "BASELINE config 4 batch: 512 independent registrations per GPU per step "
                            "(8 submaps x 64 scans), 2000-pt synthetic radar scan vs 100x100-slot 0.5 m NDT submap, "
                            "indoor parameters, NDT build + association + GNC/LM solve (estimateLoopConstraint unit)",
                "batch_per_gpu": B, "points_per_scan": N_POINTS, "submap_slots": N_SLOTS, "n_neighbours": k,
                "parameterization": "ambient4 (reference loop-closure behaviour)", "gnc_steps": mp.gnc_steps,
                "streams": n_streams,
                "mean_scan_cells": m_mean, "mean_residuals": n_res_mean, "mean_lm_iterations": float(res["iterations"].mean()),
                "mean_passes": float(res["n_evals"].mean()),
            },
            "repeats": rinfo["repeats"], "region_ms": rinfo["region_ms"],
            "region_note": "value = batch x steps / the MEDIAN of `repeats` regions of exactly `steps` steps, each between barrier + synchronize "
                           "(fill and drain of the 16-stream pipeline included: a burst figure at small --steps); `sustained` (--full) = the settle region",
            "host_enqueue_ms_per_step": t_enqueued / n_steps * 1e3,
            "stage_ms": {"ndt_build": float(stage_ms[0]), "associate": float(stage_ms[1]), "solve": float(stage_ms[2]),
                         "note": "HIP-event residency of each launch while %d batches share the chip (not a per-step cost)" % n_streams},
        }
        if multi:
            # LOUD: a first-ever RCCL failure on a multi-GPU node must not look like a pass
            out["group_fallback"] = bool(grp is None and not via_cpu)
            out["group_transport"] = "randt_group over RCCL (C ABI)" if grp is not None else ("gloo control-flow test" if via_cpu else "torch.distributed FALLBACK")
            if group_error:
                out["group_error"] = group_error
            if share_gpu:
                out["ranks_share_one_gpu"] = True   # a test of the RCCL path (socket transport between fake nodes), NOT a scaling figure
        if strong is not None:
            out["strong_scaling"] = strong
        if args.dump_outputs:
            write_outputs(args.dump_outputs, dump[0].numpy(), dump[1].numpy().view(R.RESULT_DTYPE).reshape(-1))
        if args.full:
            b_alg = algorithmic_bytes(N_POINTS, N_SLOTS, m_mean, k)
            counters, counters_file, counters_stale = load_counters()
            if "sustained" in rinfo:
                out["sustained"] = rinfo["sustained"]
            out["hbm_achieved"] = hbm_achieved(counters, elapsed / n_steps * 1e3, rinfo["sustained"]["ms_per_step"] if "sustained" in rinfo else None,
                                               counters_file, counters_stale)
            # Everything below is a side measurement on rank 0: a failure there must never cost the headline line.
            def side(key, fn, *a):
                try:
                    r = fn(*a)
                    if key is None:
                        out.update(r)
                    else:
                        out[key] = r
                except Exception as e:  # noqa: BLE001 -- reported in the line, not raised
                    out[key or "side_measurement_error"] = {"error": "%s: %s" % (type(e).__name__, e)}

            if not args.no_roofline_sections and args.only is None and args.batch_scale == 1:
                # (at N > 1 too: rank 0 alone, the other ranks wait at the closing barrier; per-GPU figures)
                side(None, roofline_sections, R, torch, full, streams, ctxs, submaps_v, mapp, clu, mp, counters, counters_file,
                     b_alg, (rinfo["sustained"]["value"] if "sustained" in rinfo else value) / world,
                     (rinfo["sustained"]["ms_per_step"] * 1e-3 if "sustained" in rinfo else elapsed / n_steps), counters_stale, throughput_mode,
                     elapsed / n_steps)
            if world == 1 and args.only is None and args.batch_scale == 1 and args.distinct_inputs > 1:
                def distinct_region():
                    # the headline once more with the point batches at DISTINCT addresses: step s reads copy s % n of the 512 scans
                    # (n x 16.4 MB > the 256 MB Infinity Cache: no step meets its input again in a cache); the working sets of the 16
                    # streams (scan cell tables, correspondences: 265 MB) were distinct all along
                    n = args.distinct_inputs
                    full.points_rotation = [full.points] + [full.points.clone() for _ in range(n - 1)]
                    try:
                        warm_up(torch, full, streams, 2 * n_streams)
                        d_steps, d_elapsed, _, _, d_last_pose, d_info = region(full)
                    finally:
                        full.points_rotation = None
                    r = {"copies": n, "input_bytes": int(n * full.points.numel() * 4), "steps": d_steps, "ms_per_step": d_elapsed / d_steps * 1e3,
                         "value": B * d_steps / d_elapsed, "unit": "registrations/s", "region_ms": d_info["region_ms"],
                         "poses_equal_headline": bool(torch.equal(d_last_pose, last_pose)),
                         "note": "same values at other addresses: identical results, nothing re-read from the Infinity Cache"}
                    if "sustained" in d_info:
                        r["sustained"] = {k: d_info["sustained"][k] for k in ("steps", "ms_per_step", "value")}
                    return r
                side("distinct_inputs", distinct_region)
            if world == 1 and args.only is None and args.batch_scale == 1 and throughput_mode and n_streams > 1 and not args.no_auto_region:
                def auto_region():
                    # the headline region with every context left in RANDT_SOLVE_AUTO: the library itself has to notice that 16 contexts
                    # keep batches in flight (enqueue stamps / hipStreamQuery) and take the throughput placement -- same rate, same poses
                    for c in ctxs:
                        c.set_solve_mode(R._capi.SOLVE_AUTO)
                    try:
                        warm_up(torch, full, streams, 2 * n_streams)
                        a_steps, a_elapsed, _, _, a_last_pose, a_info = region(full)
                    finally:
                        for c in ctxs:
                            c.set_solve_mode(R._capi.SOLVE_THROUGHPUT)
                    r = {"value": B * a_steps / a_elapsed, "unit": "registrations/s", "ms_per_step": a_elapsed / a_steps * 1e3,
                         "vs_explicit_throughput_mode": (B * a_steps / a_elapsed) / value, "poses_equal_headline": bool(torch.equal(a_last_pose, last_pose))}
                    if "sustained" in a_info:
                        r["sustained"] = {k: a_info["sustained"][k] for k in ("steps", "ms_per_step", "value")}
                        if "sustained" in rinfo:
                            r["sustained"]["vs_explicit_throughput_mode"] = a_info["sustained"]["value"] / rinfo["sustained"]["value"]
                    return r
                side("solve_auto_detection", auto_region)
            if not args.no_cpu_baseline and world == 1:
                side(None, cpu_baseline, weak_prob, mp, last_pose.cpu().numpy(), args.cpu_seconds)
            if world == 1 and args.only is None and not args.no_config2:
                side("config2_single_pair", config2_single_pair, R, torch, ctx, submaps, full, mapp, clu, mp, weak_prob, not args.no_cpu_baseline,
                     min(3.0, args.cpu_seconds))
                if throughput_mode:
                    ctx.set_solve_mode(R._capi.SOLVE_THROUGHPUT)
            if world == 1 and args.only is None and not args.no_config2:
                side("loop_gate_and_search", loop_gate_and_search, R, torch, ctx, submaps, full, mp, weak_prob, not args.no_cpu_baseline, min(2.0, args.cpu_seconds))
            if args.odometry_scans > 0 and world == 1:
                side("config3_streaming_odometry", streaming_odometry, ctx, args.odometry_scans, not args.no_cpu_baseline)
            if args.replica_steps > 0 and world == 1:
                side("config3_replicas", config3_replicas, ctx, args.replica_steps)
            if args.cpp_drive_scans > 0 and world == 1:
                py = out.get("config3_streaming_odometry", {})
                side("cpp_local_fuser_drive", cpp_local_fuser_drive, ctx, args.cpp_drive_scans, py.get("ms_per_scan") if isinstance(py, dict) else None)
            if args.polar_scans > 0 and world == 1:
                side("config5_polar_filter", polar_filter, ctx, args.polar_scans)
            if args.slam_scans > 0 and world == 1:
                side("slam_loop", slam_loop, ctx, args.slam_scans)
            if args.polar_odometry_scans > 0 and world == 1:
                side("config5_polar_odometry", polar_odometry, ctx, args.polar_odometry_scans)
        print(json.dumps(out))
    if multi:
        dist.barrier()
        dist.destroy_process_group()


def roofline_sections(R, torch, full, streams, ctxs, submaps_v, mapp, clu, mp, counters, counters_file, b_alg, value, s_per_step, counters_stale=None, throughput_mode=True,
                      headline_s_per_step=None):
    """Clean (non-overlapped) measurements behind the `roofline` object, all with HIP events on the launch stream:
      single_batch      ONE 512-registration batch at a time on one stream: latency, rate, per-kernel durations;
      chip-filling      the dominant kernel (k_solve) with SAT_COPIES copies of the batch = 8192 registrations in ONE
                        launch, one stream: the launch fills the chip by itself, so its duration is a per-launch cost and
                        the rocprofv3 kernel trace of the same command shows the same number."""
    st, B = streams[0], full.B
    # ---- single batch, single stream: the library's own choice of solve geometry (RANDT_SOLVE_AUTO)
    ctxs[0].set_solve_mode(R._capi.SOLVE_AUTO)
    reps = 200
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    poses = [full.guess4.clone() for _ in range(reps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        full.step(0, st, poses[i], ev[i])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    sb = np.array([[ev[s][i].elapsed_time(ev[s][i + 1]) for i in range(3)] for s in range(reps)]).mean(axis=0) * 1e3   # us
    lat = np.array([ev[s][0].elapsed_time(ev[s][3]) for s in range(reps)]).mean() * 1e3
    single = {"streams": 1, "registrations_per_launch": B, "value": B * reps / el, "unit": "registrations/s",
              "batch_latency_us": float(lat),
              "kernel_us": {"k_ndt_build": float(sb[0]), "k_associate": float(sb[1]), "k_solve": float(sb[2])},
              "note": "one 512-registration batch alone (a loop-closure burst), solve geometry chosen by the library "
                      "(RANDT_SOLVE_AUTO: eight wavefronts per registration at this size)"}
    # the per-GPU share of an 8-GPU split of the same batch: 64 registrations alone on the device
    sub = Batch(R, torch, ctxs[:1], submaps_v[:1], mapp, clu, mp, full.points[:64].contiguous(), full.fixed_idx[:64].contiguous(),
                full.guess4[:64].contiguous())
    ev64 = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    p64 = [sub.guess4.clone() for _ in range(reps)]
    for i in range(3):
        sub.step(0, st, sub.poses[0])
    torch.cuda.synchronize()
    for i in range(reps):
        sub.step(0, st, p64[i], ev64[i])
    torch.cuda.synchronize()
    sb64 = np.array([[ev64[s][i].elapsed_time(ev64[s][i + 1]) for i in range(3)] for s in range(reps)]).mean(axis=0) * 1e3
    single["batch_of_64"] = {"batch_latency_us": float(np.array([ev64[s][0].elapsed_time(ev64[s][3]) for s in range(reps)]).mean() * 1e3),
                             "kernel_us": {"k_ndt_build": float(sb64[0]), "k_associate": float(sb64[1]), "k_solve": float(sb64[2])}}
    sub.scan_maps[0].close()
    # ---- chip-filling launch of the dominant kernel
    rep = lambda t: t.repeat(*([SAT_COPIES] + [1] * (t.dim() - 1))).contiguous()
    big = Batch(R, torch, ctxs[:1], submaps_v[:1], mapp, clu, mp, rep(full.points), rep(full.fixed_idx), rep(full.guess4))
    big.step(0, st, big.poses[0])                       # build + associate (+ a warm-up solve) once
    n_l = 20
    bp = [big.guess4.clone() for _ in range(n_l)]
    e0 = [torch.cuda.Event(enable_timing=True) for _ in range(n_l)]
    e1 = [torch.cuda.Event(enable_timing=True) for _ in range(n_l)]
    e_b = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    for i in range(n_l):
        e0[i].record(st)
        R.solve_batch(ctxs[0], submaps_v[0], big.fixed_idx, big.scan_maps[0], 0, big.B, big.corrs[0], mp, bp[i], big.results[0])
        e1[i].record(st)
    e_b[0].record(st)
    R.ndt_build_batch(ctxs[0], big.points, clu, big.scan_maps[0])
    e_b[1].record(st)
    R.associate_batch(ctxs[0], submaps_v[0], big.fixed_idx, big.scan_maps[0], 0, big.B, big.guess4, mp, big.corrs[0])
    e_b[2].record(st)
    torch.cuda.synchronize()
    sat_us = float(np.mean([e0[i].elapsed_time(e1[i]) for i in range(n_l)]) * 1e3)
    sat_build_us, sat_assoc_us = e_b[0].elapsed_time(e_b[1]) * 1e3, e_b[1].elapsed_time(e_b[2]) * 1e3

    ks = counters.get("k_solve<3,1,64,true,4,false>")
    roof = {"bound": "valu_issue", "unit": "G SIMD-cycles/s", "peak": VALU_PEAK,
            "peak_note": "%d SIMDs x %.1f GHz max clock; one wave64 VALU instruction occupies its SIMD's issue port for the spec "
                         "cycles listed in cycle_costs (fp32-class 2, fp64 4 = the 78.6 TFLOP/s vector-fp64 rate, transcendental 8 / 16; "
                         "tools/clock_probe.hip measures 0.88-0.97 of these rates at a 2.1-2.4 GHz shader clock)" % (N_SIMDS, CLOCK_GHZ),
            "kernel": "k_solve<3,1,64,true,4,false> (dominant: 62 % of the path's VALU issue cycles)",
            "launch": "%d registrations (%d copies of the 512 batch) in ONE launch, one stream, nothing else running" % (big.B, SAT_COPIES),
            "avg_launch_us": sat_us, "achieved": None, "frac": None, "traffic": None, "counters": counters_file}
    if counters_stale:
        roof["counters_refused"] = counters_stale
    out = {"roofline": roof, "single_batch": single}
    if ks is not None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from pmc_summary import VALU_COST

        cyc = {n: counters[n]["valu_issue_cycles"] for n in counters}            # per 512-registration launch
        cyc_l = ks["valu_issue_cycles"] * SAT_COPIES
        roof.update({
            "valu_issue_cycles_per_launch": cyc_l,
            "achieved": cyc_l / sat_us * 1e-3, "frac": cyc_l / sat_us * 1e-3 / VALU_PEAK,
            "cycle_costs": VALU_COST,
            "counted_per_512_launch": {c: ks[c] for c in ("SQ_INSTS_VALU", "SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64",
                                                          "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_TRANS_F64", "SQ_ACTIVE_INST_VALU") if c in ks},
            # HBM bytes per launch from the TCC counters: FETCH_SIZE KB x2 (gfx950 correction) + WRITE_SIZE KB
            "traffic": int((2.0 * ks.get("FETCH_SIZE", 0.0) + ks.get("WRITE_SIZE", 0.0)) * 1024 * SAT_COPIES),
            "traffic_note": "PMC bytes of one launch (FETCH_SIZE x2 per the gfx950 note + WRITE_SIZE, scaled from the 512-registration "
                            "launch); ~10x below the SURVEY byte model: the path is not HBM-bound",
            "instructions_per_registration": ks["SQ_INSTS_VALU"] / 512.0,
            "single_stream_512_launch": {"avg_launch_us": float(sb[2]), "frac": ks["valu_issue_cycles"] / float(sb[2]) * 1e-3 / VALU_PEAK,
                                         "note": "512 wavefronts on 1024 SIMDs: at most half the chip, one wavefront per SIMD"},
        })
        if all(n in cyc for n in HOT_KERNELS):
            tot = sum(cyc[n] for n in HOT_KERNELS)
            roof["path"] = {
                "valu_issue_cycles_per_step": tot, "by_kernel": {n: cyc[n] for n in HOT_KERNELS},
                # the headline's OWN step time (exactly --steps steps between synchronisations: fill and drain of the pipeline are in
                # it), and the sustained step beside it
                "achieved": tot / ((headline_s_per_step or s_per_step) * 1e6) * 1e-3,
                "frac": tot / ((headline_s_per_step or s_per_step) * 1e6) * 1e-3 / VALU_PEAK,
                "ms_per_step": (headline_s_per_step or s_per_step) * 1e3,
                "sustained": {"ms_per_step": s_per_step * 1e3, "achieved": tot / (s_per_step * 1e6) * 1e-3, "frac": tot / (s_per_step * 1e6) * 1e-3 / VALU_PEAK},
                "note": "all three launches of a step / ms_per_step of the headline region (`sustained`: of the settle region: the steady "
                        "rate of the 16-stream pipeline; throughput, no residency involved)",
                "chip_filling_launch_us": {"k_ndt_build": sat_build_us, "k_associate": sat_assoc_us, "k_solve": sat_us,
                                           "registrations": big.B},
                # each kernel by itself: issue cycles of its chip-filling launch / that launch's duration (the two short kernels are
                # chains of LDS atomics / L2 round trips: their chip time, not their issue slots, is what the pipelined region overlaps)
                "frac_by_kernel": {n: cyc[n] * SAT_COPIES / us * 1e-3 / VALU_PEAK
                                   for n, us in zip(HOT_KERNELS, (sat_build_us, sat_assoc_us, sat_us))},
            }
        flops = ks["fp64_flops"]
        out["roofline_fp64"] = {"bound": "fp64_valu", "kernel": "k_solve", "unit": "TFLOP/s", "peak": FP64_PEAK_TFLOPS,
                                "achieved": flops * SAT_COPIES / sat_us * 1e-6, "frac": flops * SAT_COPIES / sat_us * 1e-6 / FP64_PEAK_TFLOPS,
                                "flops_per_registration": flops / 512.0,
                                "note": "EXECUTED fp64 flops from SQ_INSTS_VALU_{FMA x2, MUL, ADD, TRANS}_F64 x 64 lanes (redundant all-lane "
                                        "LM algebra included), chip-filling launch"}
    out["roofline_hbm_secondary"] = {
        "bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "algorithmic_bytes_per_registration": b_alg,
        "path_effective": {"achieved": value * b_alg / 1e9, "frac": value * b_alg / 1e9 / HBM_PEAK_GBS},
        "note": "SURVEY 8(d) byte model (counts the dense 480 KB submap table once per registration) x registrations/s; kept for "
                "continuity with round 1 -- the compact cell tables make the real traffic ~10x smaller, see roofline.traffic"}
    big.scan_maps[0].close()
    if throughput_mode:
        ctxs[0].set_solve_mode(R._capi.SOLVE_THROUGHPUT)
    # ---- the dominant kernel SUSTAINED: the 512-registration solve launches of all streams back to back (what the kernel does
    # when the tail of one launch is covered by the next ones; the single chip-filling launch above pays its own tail)
    if ks is not None and throughput_mode and len(streams) > 1 and len(full.ctxs) >= len(streams):
        n_s, per = len(streams), 96
        sp = [[full.guess4.clone() for _ in range(per)] for _ in range(n_s)]
        for j in range(n_s):                                   # (the streams' correspondence tables are those of the headline region)
            full.step(j, streams[j], full.poses[j], None, "solve")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(per):
            for j in range(n_s):
                full.step(j, streams[j], sp[j][i], None, "solve")
        torch.cuda.synchronize()
        us_512 = (time.perf_counter() - t0) / (per * n_s) * 1e6
        roof["sustained"] = {"us_per_512_launch": us_512, "achieved": ks["valu_issue_cycles"] / us_512 * 1e-3,
                             "frac": ks["valu_issue_cycles"] / us_512 * 1e-3 / VALU_PEAK,
                             "note": "%d x %d launches of the 512-registration solve on %d streams, wall clock between synchronisations "
                                     "(nothing else running): the same kernel with its launch tails covered" % (per, n_s, n_s)}
    return out


def config2_single_pair(R, torch, ctx, submaps, full, mapp, clu, mp, prob, with_cpu, budget_s):
    """BASELINE config 2 as a caller feels it (LocalFuser calls estimateLoopConstraint one candidate at a time,
    local_fuser.cpp:335,387,395): host call -> result latency of ONE registration on an otherwise idle GPU, through
    (a) randt_register_pair (maps resident, host pose in / out, synchronous) and (b) randt_scan_register_batch_dev with B = 1
    (raw scan resident, NDT build + association + solve, then a stream synchronisation), with the HIP-event kernel share of (b);
    beside them the CPU oracle on the same pair at one thread and with its residual blocks over all granted cores (what
    Ceres' num_threads = hardware_concurrency() does, ndt_matcher.cpp:376,461)."""
    from randt_slam_amd import host

    dev = full.points.device
    st = torch.cuda.current_stream()
    ctx.set_solve_mode(R._capi.SOLVE_AUTO)
    pts = full.points[:1].contiguous()
    fidx = full.fixed_idx[:1].contiguous()
    g4 = full.guess4[:1].contiguous()
    sub_i = int(fidx[0].item())
    ws = R.Maps(ctx, 1, mapp, 512, with_grid=False)
    res = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
    reps = 300
    lat_b, ker_b = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(reps + 20):
        pose = g4.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        R.scan_register_batch(ctx, pts, clu, submaps, fidx, ws, mp, pose, res)
        e1.record(st)
        ctx.synchronize()
        t1 = time.perf_counter()
        if i >= 20:
            lat_b.append((t1 - t0) * 1e6)
            ker_b.append(e0.elapsed_time(e1) * 1e3)
    g_host = g4.cpu().numpy()[0]
    lat_a = []
    for i in range(reps + 20):
        t0 = time.perf_counter()
        p_a, r_a = host.register_pair(ctx, submaps, sub_i, ws, 0, mp, g_host)
        t1 = time.perf_counter()
        if i >= 20:
            lat_a.append((t1 - t0) * 1e6)
    q = lambda v: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)), "calls": len(v)}
    out = {"workload": "ONE 2000-point scan against ONE 100x100-slot submap (registration 0 of the config-4 batch), GPU otherwise idle",
           "randt_register_pair": dict(q(lat_a), note="scan cells already built and resident; host pose in, pose + record out, synchronous"),
           "randt_scan_register_batch_dev_B1": dict(q(lat_b), kernel_us_hip_events=float(np.median(ker_b)),
                                                    note="raw scan resident; NDT build + association + solve (split geometry, eight wavefronts) "
                                                         "+ one stream synchronisation; kernel_us = first launch to last launch end on the stream"),
           "iterations": int(r_a["iterations"]), "n_residuals": int(r_a["n_residuals"])}
    ws.close()
    if with_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle as po
        from randt_slam_amd import synth

        ip = synth.indoor_params()
        mk = lambda cap=None: po.Map(ip["size_x"], ip["size_y"], ip["resolution"], (0, 0), ip["max_neighbour_dist"], ip["min_points_per_cell"], cap)
        sm = prob["submaps"][sub_i]
        osub = mk()
        for t in range(len(sm["kf_scans"])):
            m = mk(512)
            m.build(sm["kf_scans"][t], ip["n_clusters"], ip["max_range"])
            m.transform(synth.pose3_to_pose4(sm["kf_rel"][t]))
            osub.merge(m)
        op = po.default_params()
        for name, _ in mp._fields_:
            if name != "reserved":
                setattr(op, name, getattr(mp, name))
        eff, logical, quota = effective_cpus()
        cores = max(1, min(po.num_threads(), eff))
        g0 = synth.pose3_to_pose4(prob["guess"])[0]

        def leg(threads):
            po.set_eval_threads(threads)
            v, t_total, p4 = [], 0.0, None
            try:
                while t_total < budget_s or len(v) < 5:
                    t0 = time.perf_counter()
                    om = mk(512)
                    om.build(prob["scans"][0], ip["n_clusters"], ip["max_range"])
                    rc, p4, cost, stt = po.register_pair(osub, om, op, g0)
                    dt = time.perf_counter() - t0
                    v.append(dt * 1e6)
                    t_total += dt
            finally:
                po.set_eval_threads(1)
            return v, p4

        v1, p1 = leg(1)
        vn, pn = leg(cores)
        out["cpu_oracle"] = {"kind": "port", "one_thread": dict(q(v1), cores=1),
                             "residual_parallel": dict(q(vn), cores=cores,
                                                       note="OpenMP over the residual blocks of the ONE problem (timing only: the cost is then "
                                                            "a reduction in another order than the oracle proper)"),
                             "sample": "NDT build + association + GNC/LM solve of the same pair, repeated for %.0f s per leg" % budget_s,
                             "pose_vs_gpu_max_abs": float(np.abs(np.asarray(p1) - np.asarray(p_a)).max())}
    return out


def loop_gate_and_search(R, torch, ctx, submaps, full, mp, prob, with_cpu, budget_s):
    """SURVEY rows f-2 and f-3 as measurements (the two steps around a loop registration, local_fuser.cpp:329-340, 387-402):
    (f-2) Map::calculateCSDivergence for the whole config-4 batch -- 512 scans, each against its own submap at its registered
    pose: one launch, HIP events; beside it the CPU oracle on a bounded sample;
    (f-3) Matcher::estimateTransformGlobalBNB: the batched cost kernel on 4096 candidate poses of one pair, and one whole
    search from a pose 1.1 m / 0.1 rad off (host call -> result); the CPU oracle's search beside it."""
    from randt_slam_amd import host, synth

    dev = full.points.device
    st = torch.cuda.current_stream()
    B, n_sub = full.B, submaps.n_maps if hasattr(submaps, "n_maps") else int(prob["submap_of"].max()) + 1
    scan_maps = full.scan_maps[0]
    R.ndt_build_batch(ctx, full.points, full.clu, scan_maps)
    pose = torch.from_numpy(synth.pose3_to_pose4(prob["truth"])).to(dev)
    out_v = torch.zeros(B, dtype=torch.float64, device=dev)
    terms = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_cs = []
    for i in range(25):
        e0.record(st)
        host.cs_divergence_batch(ctx, submaps, 0, n_sub, full.fixed_idx, scan_maps, 0, B, pose, out_v, terms)
        e1.record(st)
        torch.cuda.synchronize()
        if i >= 5:
            t_cs.append(e0.elapsed_time(e1) * 1e-3)
    t_cs = float(np.median(t_cs))
    n_moving = scan_maps.counts().astype(np.int64)
    n_fixed_sub = submaps.counts().astype(np.int64)
    n_fixed = n_fixed_sub[prob["submap_of"]]
    # interaction per pair + the self terms (ndt_map.cpp:42-99; symmetric halves): the moving one per scan, the fixed one ONCE per
    # submap (it does not depend on the pair: k_cs_self) -- the reference, called pair by pair, evaluates it for every pair
    overlaps = int((n_fixed * n_moving).sum() + (n_fixed_sub * n_fixed_sub).sum() // 2 + (n_moving * n_moving).sum() // 2)
    overlaps_ref = int((n_fixed * n_moving).sum() + (n_fixed * n_fixed).sum() + (n_moving * n_moving).sum())
    r = {"f2_cs_divergence": {"pairs_per_launch": B, "us_per_launch": t_cs * 1e6, "pairs_per_sec": B / t_cs, "gaussian_overlaps_evaluated": overlaps,
                              "overlaps_per_sec": overlaps / t_cs, "gaussian_overlaps_in_the_reference_loops": overlaps_ref, "mean_value": float(out_v.mean().item()),
                              "below_loop_closure_gate_3.6": int((out_v < 3.6).sum().item())}}
    # f-3: cost batch + one search
    mpb = mp
    g1 = full.guess4[:1].contiguous()
    corr = torch.full((1, 512, mp.n_neighbours), -1, dtype=torch.int32, device=dev)
    R.associate_batch(ctx, submaps, full.fixed_idx[:1].contiguous(), scan_maps, 0, 1, g1, mp, corr)
    sub0 = int(full.fixed_idx[0].item())
    rng = np.random.default_rng(5)
    n_poses = 4096
    poses = torch.from_numpy(synth.pose3_to_pose4(prob["truth"][0] + rng.normal(0, [0.5, 0.5, 0.1], (n_poses, 3)))).to(dev)
    cost = torch.zeros(n_poses, dtype=torch.float64, device=dev)
    nres = torch.zeros(1, dtype=torch.int32, device=dev)
    t_ev = []
    for i in range(25):
        e0.record(st)
        host.eval_cost_batch(ctx, submaps, sub0, scan_maps, 0, corr, mp, 1.5, poses, cost, nres)
        e1.record(st)
        torch.cuda.synchronize()
        if i >= 5:
            t_ev.append(e0.elapsed_time(e1) * 1e-3)
    t_ev = float(np.median(t_ev))
    bad = synth.pose3_to_pose4(prob["truth"][0] + np.array([0.9, -0.7, 0.1]))
    bp = host.bnb_params(cost_threshold=2.0)
    lat = []
    for i in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc, t4, ne = host.search_global(ctx, submaps, sub0, scan_maps, 0, mp, bp, bad)
        lat.append(time.perf_counter() - t0)
    t_search = float(np.median(lat[2:]))
    est = synth.pose4_to_pose3(t4)
    r["f3_global_search"] = {"cost_batch": {"poses": n_poses, "residuals_per_pose": int(nres.item()), "us_per_launch": t_ev * 1e6,
                                            "pose_evaluations_per_sec": n_poses / t_ev, "residual_evaluations_per_sec": n_poses * int(nres.item()) / t_ev},
                             "search": {"ms_per_search": t_search * 1e3, "cost_evaluations": int(ne), "min_cost": float(mc),
                                        "error_vs_truth_m": float(np.hypot(*(est[:2] - prob["truth"][0][:2])))}}
    if with_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle as po

        ip = synth.indoor_params()

        def omap(cap=None):
            return po.Map(ip["size_x"], ip["size_y"], ip["resolution"], (0, 0), ip["max_neighbour_dist"], ip["min_points_per_cell"], cap)
        sm = prob["submaps"][int(prob["submap_of"][0])]
        osub = omap()
        for t in range(len(sm["kf_scans"])):
            m = omap(512)
            m.build(sm["kf_scans"][t], ip["n_clusters"], ip["max_range"])
            m.transform(synth.pose3_to_pose4(sm["kf_rel"][t]))
            osub.merge(m)
        idx = [i for i in range(B) if prob["submap_of"][i] == prob["submap_of"][0]][:16]
        oscans = []
        for i in idx:
            m = omap(512)
            m.build(prob["scans"][i], ip["n_clusters"], ip["max_range"])
            m.transform(synth.pose3_to_pose4(prob["truth"][i]))
            oscans.append(m)
        done, t_tot, worst = 0, 0.0, 0.0
        gv = out_v.cpu().numpy()
        while t_tot < budget_s:
            t0 = time.perf_counter()
            vals = [po.cs_divergence(osub, m)[0] for m in oscans]
            t_tot += time.perf_counter() - t0
            done += len(oscans)
        worst = float(np.abs(np.array(vals) - gv[idx]).max())
        r["f2_cs_divergence"]["cpu_oracle"] = {"pairs_per_sec": done / t_tot, "cores": 1, "sample": "%d pairs of submap %d, repeated for %.1f s" % (len(idx), int(prob["submap_of"][0]), t_tot),
                                              "max_abs_difference_vs_gpu": worst}
        oscan0 = omap(512)
        oscan0.build(prob["scans"][0], ip["n_clusters"], ip["max_range"])
        op = po.default_params()
        for name, _ in mp._fields_:
            if name != "reserved":
                setattr(op, name, getattr(mp, name))
        t0 = time.perf_counter()
        omc, ot4, one = po.search_global_bnb(osub, oscan0, op, po.bnb_params(cost_threshold=2.0), bad)
        t_o = time.perf_counter() - t0
        r["f3_global_search"]["cpu_oracle"] = {"ms_per_search": t_o * 1e3, "cores": 1, "cost_evaluations": int(one),
                                               "same_result": bool(one == ne and np.array_equal(ot4, t4))}
    return r


def polar_filter(ctx, n_scans):
    """BASELINE config 5 front end (side measurement): RadarPreprocessor::filterScan on Oxford-shaped
    polar scans, 400 azimuths x 3000 bins x 16 B = 19.2 MB per scan read once -> the one genuinely
    HBM-streaming stage of the path; followed by the NDT build of the filtered points."""
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import host, synth

    dev = torch.device("cuda", ctx.device)
    world = synth.make_world()
    tr = synth.make_trajectory(3400, 4)
    base = [torch.from_numpy(synth.make_polar_scan(world, tr[i], 70 + i)).to(dev) for i in range(4)]
    raw = torch.stack([base[i % 4] for i in range(n_scans)]).contiguous()      # distinct HBM copies
    pitch = 6144
    out = torch.zeros((n_scans, pitch, 4), dtype=torch.float32, device=dev)
    counts = torch.zeros(n_scans, dtype=torch.int32, device=dev)
    status = torch.zeros(n_scans, dtype=torch.int32, device=dev)
    fp = host.filter_params()
    maps = R.Maps(ctx, n_scans, R.indoor_map_params(), 1024, with_grid=False)
    st = torch.cuda.current_stream()
    for _ in range(2):
        host.filter_scan_batch(ctx, raw, fp, out, counts, status)
        R.ndt_build_batch(ctx, out, R.indoor_cluster_params(), maps, n_points=counts)
    torch.cuda.synchronize()
    reps = 10
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_f = t_b = 0.0
    for _ in range(reps):
        e[0].record(st)
        host.filter_scan_batch(ctx, raw, fp, out, counts, status)
        e[1].record(st)
        R.ndt_build_batch(ctx, out, R.indoor_cluster_params(), maps, n_points=counts)
        e[2].record(st)
        torch.cuda.synchronize()
        t_f += e[0].elapsed_time(e[1])
        t_b += e[1].elapsed_time(e[2])
    t_f, t_b = t_f / reps * 1e-3, t_b / reps * 1e-3
    nbytes = raw.numel() * 4
    # the stage as a stream of launches: 20 launches back to back over FOUR distinct input buffers (1.2 GB: nothing of a
    # launch's input is still in the 256 MB Infinity Cache when its buffer comes round again), one event pair around them
    t_bb = None
    if n_scans == 16:
        raws = [raw] + [raw.clone() for _ in range(3)]
        for r in raws:
            host.filter_scan_batch(ctx, r, fp, out, counts, status)
        torch.cuda.synchronize()
        e[0].record(st)
        for i in range(20):
            host.filter_scan_batch(ctx, raws[i % 4], fp, out, counts, status)
        e[1].record(st)
        torch.cuda.synchronize()
        t_bb = e[0].elapsed_time(e[1]) / 20 * 1e-3
        # the same 20 launches dealt to TWO contexts / streams in turn (a caller replaying a bag keeps two batches in flight): the
        # emission of one launch -- a 5.6 us dependent tail on 16 workgroups -- and its fill / drain overlap the next launch's rows
        t_2s = None
        try:
            side = torch.cuda.Stream(device=dev)
            ctx2 = R.Context(ctx.device, side.cuda_stream)
            out2, counts2, status2 = torch.zeros_like(out), torch.zeros_like(counts), torch.zeros_like(status)
            host.filter_scan_batch(ctx2, raws[1], fp, out2, counts2, status2)
            torch.cuda.synchronize()
            e[0].record(st)
            side.wait_event(e[0])
            for i in range(20):
                if i % 2 == 0:
                    host.filter_scan_batch(ctx, raws[i % 4], fp, out, counts, status)
                else:
                    host.filter_scan_batch(ctx2, raws[i % 4], fp, out2, counts2, status2)
            st.wait_stream(side)
            e[1].record(st)
            torch.cuda.synchronize()
            t_2s = e[0].elapsed_time(e[1]) / 20 * 1e-3
            two_ok = bool((status2 == 0).all().item()) and bool((counts2 == counts).all().item())   # raws[3] last on both: same scans, same counts
            del out2, ctx2
        except Exception as ex:  # noqa: BLE001 -- a side measurement
            t_2s, two_ok = None, "%s" % ex
        del raws
    # the same stage with 64 scans per launch (1.23 GB of input: nothing of it is still in the Infinity Cache when it is read):
    # the fill and drain of a launch and the emission are paid once per 64 scans instead of once per 16
    long_launch = None
    if n_scans == 16:
        raw64 = torch.cat([raw, raw, raw, raw]).contiguous()
        out64 = torch.zeros((64, pitch, 4), dtype=torch.float32, device=dev)
        counts64 = torch.zeros(64, dtype=torch.int32, device=dev)
        status64 = torch.zeros(64, dtype=torch.int32, device=dev)
        for _ in range(2):
            host.filter_scan_batch(ctx, raw64, fp, out64, counts64, status64)
        torch.cuda.synchronize()
        t64 = []
        for _ in range(5):
            e[0].record(st)
            host.filter_scan_batch(ctx, raw64, fp, out64, counts64, status64)
            e[1].record(st)
            torch.cuda.synchronize()
            t64.append(e[0].elapsed_time(e[1]) * 1e-3)
        t64 = sorted(t64)[2]
        long_launch = {"scans_per_launch": 64, "ms": t64 * 1e3, "achieved": 4 * nbytes / t64 / 1e9, "frac": 4 * nbytes / t64 / 1e9 / HBM_PEAK_GBS,
                       "status_ok": bool((status64 == 0).all().item()), "same_counts": bool((counts64.view(4, 16) == counts.view(1, 16)).all().item())}
        del raw64, out64
    # ONE scan per launch -- what the online node runs (a 4 Hz sensor hands over one scan at a time): (a) a lone launch between
    # two host synchronisations, median of 30, each over another of the 16 distinct scans; (b) the same launches as a chain of 64
    single_scan = None
    if n_scans >= 2:
        o1 = torch.zeros((1, pitch, 4), dtype=torch.float32, device=dev)
        c1 = torch.zeros(1, dtype=torch.int32, device=dev)
        s1 = torch.zeros(1, dtype=torch.int32, device=dev)
        for i in range(n_scans):
            host.filter_scan_batch(ctx, raw[i:i + 1], fp, o1, c1, s1)
        torch.cuda.synchronize()
        lone = []
        for i in range(30):
            e[0].record(st)
            host.filter_scan_batch(ctx, raw[i % n_scans:i % n_scans + 1], fp, o1, c1, s1)
            e[1].record(st)
            torch.cuda.synchronize()
            lone.append(e[0].elapsed_time(e[1]) * 1e-3)
        t1 = float(np.median(lone))
        e[0].record(st)
        for i in range(64):
            host.filter_scan_batch(ctx, raw[i % n_scans:i % n_scans + 1], fp, o1, c1, s1)
        e[1].record(st)
        torch.cuda.synchronize()
        tc = e[0].elapsed_time(e[1]) / 64 * 1e-3
        b1 = nbytes // n_scans
        single_scan = {"us": t1 * 1e6, "achieved": b1 / t1 / 1e9, "frac": b1 / t1 / 1e9 / HBM_PEAK_GBS,
                       "chain_us_per_launch": tc * 1e6, "chain_frac": b1 / tc / 1e9 / HBM_PEAK_GBS, "bytes": b1,
                       "same_count_as_batched": bool(int(c1.item()) == int(counts[63 % n_scans].item())), "status_ok": bool(int(s1.item()) == 0),
                       "note": "k_filter_rows + k_filter_emit of ONE 400 x 3000 scan (19.2 MB), HIP events; a kernel of this shape that only loads "
                               "takes 5.6 us launched alone (tools/filter_ticket_probe.hip: 0.43 of 8 TB/s is what one scan per launch can reach)"}
    roof = {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "achieved": nbytes / t_f / 1e9, "frac": nbytes / t_f / 1e9 / HBM_PEAK_GBS,
            "algorithmic_bytes": nbytes, "traffic": None,
            "note": "f-1 stage end to end (k_filter_rows + k_filter_emit, HIP events on the launch stream): raw polar bytes read once / duration "
                    "of ONE launch between two host synchronisations; back_to_back: the same launch as a stream of 20 over four distinct inputs; "
                    "long_launch: 64 scans (1.23 GB) in one launch"}
    if single_scan:
        roof["single_scan"] = single_scan
    if long_launch:
        roof["long_launch"] = long_launch
    if t_bb:
        roof["back_to_back"] = {"ms": t_bb * 1e3, "achieved": nbytes / t_bb / 1e9, "frac": nbytes / t_bb / 1e9 / HBM_PEAK_GBS, "launches": 20, "distinct_inputs": 4}
        if t_2s:
            roof["two_streams"] = {"ms": t_2s * 1e3, "achieved": nbytes / t_2s / 1e9, "frac": nbytes / t_2s / 1e9 / HBM_PEAK_GBS, "launches": 20, "distinct_inputs": 4,
                                   "streams": 2, "same_counts": two_ok,
                                   "note": "the back_to_back launches dealt to two contexts in turn: one launch's emission and drain run beside the next one's rows"}
    # counter rows of the two kernels at THIS launch size (a workgroup of 256 threads per row; 512 threads per scan)
    fr, fe = find_row("k_filter_rows<true,true>", n_scans * 400 * 256), find_row("k_filter_emit<true>", n_scans * 512)
    fr1, fe1 = find_row("k_filter_rows<true,true>", 400 * 256), find_row("k_filter_emit<true>", 512)
    if single_scan and fr1 and fe1 and fr1.get("single_stream_avg_us") and fe1.get("single_stream_avg_us"):
        us = float(fr1["single_stream_avg_us"]) + float(fe1["single_stream_avg_us"])
        single_scan["rocprof_avg_us"] = {"k_filter_rows": float(fr1["single_stream_avg_us"]), "k_filter_emit": float(fe1["single_stream_avg_us"])}
        single_scan["rocprof_frac"] = single_scan["bytes"] / (us * 1e-6) / 1e9 / HBM_PEAK_GBS   # bytes / (rocprofv3 durations of the two kernels) / 8 TB/s
    if fr and fe and n_scans == 16:
        # HBM bytes from the TCC counters of the committed summary (FETCH_SIZE KB x2 per the gfx950 note + WRITE_SIZE KB), both kernels
        roof["traffic"] = int((2.0 * (fr.get("FETCH_SIZE", 0.0) + fe.get("FETCH_SIZE", 0.0)) + fr.get("WRITE_SIZE", 0.0) + fe.get("WRITE_SIZE", 0.0)) * 1024)
        # the counted bytes (not the algorithmic ones) over the same launch duration
        roof["hbm_achieved"] = {"bytes_per_launch": roof["traffic"], "achieved": roof["traffic"] / t_f / 1e9, "frac": roof["traffic"] / t_f / 1e9 / HBM_PEAK_GBS}
        if fr.get("single_stream_avg_us"):
            roof["rocprof_avg_us"] = {"k_filter_rows": fr.get("single_stream_avg_us"), "k_filter_emit": fe.get("single_stream_avg_us")}
            roof["k_filter_rows_frac"] = nbytes / (float(fr["single_stream_avg_us"]) * 1e-6) / 1e9 / HBM_PEAK_GBS
            # the round-3 verdict's definition of this stage's line: bytes / (rocprofv3 durations of the two kernels) / 8 TB/s
            roof["rocprof_frac"] = nbytes / ((float(fr["single_stream_avg_us"]) + float(fe["single_stream_avg_us"])) * 1e-6) / 1e9 / HBM_PEAK_GBS
    return {"roofline": roof, "scans_per_launch": n_scans, "raw_bytes_per_scan": nbytes // n_scans, "filter_ms": t_f * 1e3, "ndt_build_ms": t_b * 1e3,
            "filter_GBps": nbytes / t_f / 1e9, "filter_hbm_frac": nbytes / t_f / 1e9 / HBM_PEAK_GBS,
            "scans_per_sec_filter_plus_build": n_scans / (t_f + t_b), "mean_filtered_points": float(counts.float().mean().item()),
            "status_ok": bool((status == 0).all().item())}


def slam_loop(ctx, n_scans):
    """Side measurement: the reference's whole SLAM loop as a call pattern (randt_slam_amd/slam.py) -- fixed-lag odometry
    with submap roll-overs, graph nodes / edges, Scan Context candidates, loop registration against finished submaps, CS
    gate, pose-graph optimisation every 40 scans -- on a circular two-lap drive (160 scans per lap, 40-state submaps)."""
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import odometry, slam, synth

    world = synth.make_world()
    dt, per_lap = 0.25, 160
    th = 2 * np.pi * np.arange(n_scans) / per_lap
    truth = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    scans = np.stack([synth.make_scan(world, truth[i], 71000 + i) for i in range(n_scans)])
    d_scans = torch.from_numpy(scans).to(torch.device("cuda", ctx.device))
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    loop_mp = R.default_matcher_params(gnc_steps=2)
    wp = R.window_params()

    def run():
        s = slam.Slam(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params(), scan_slots=n_scans // 4 + 64,
                                          submap_slots=n_scans // 40 + 8), mp, wp, loop_mp,
                      params=dict(submap_size_poses=40, submap_overlap=10), sc_params=dict(max_radius=20.0, dist_thresh=0.5),
                      loop_closure_weight=40.0)
        t_loop = t_pg = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_scans):
            pose = s.process_scan(d_scans[i], i * dt)
            t1 = time.perf_counter()
            s.detect_loop_closures()
            t2 = time.perf_counter()
            if i % 40 == 39:
                s.optimize_pose_graph()
            t_loop += t2 - t1
            t_pg += time.perf_counter() - t2
        torch.cuda.synchronize()
        return s, pose, time.perf_counter() - t0, t_loop, t_pg

    run()                                                    # warm-up pass
    s, pose, el, t_loop, t_pg = run()
    rel = synth.se2_mul3(synth.se2_inv3(truth[0]), truth[-1])
    est = synth.pose4_to_pose3(pose)
    loops = [e for e in s.edges if e[0] + 1 != e[1]]
    # the same loop driven from C++ through the facade (tests/cpp/local_fuser_drive.cpp --slam: host buffers, Maps by value, SCManager,
    # Matcher::estimateLoopConstraint, Map::calculateCSDivergence, GlobalFuser); tests/test_gpu_local_fuser_cpp.py holds its graph to this one
    cpp = None
    try:
        import subprocess
        import tempfile

        libdir = os.path.join(ROOT, "randt-slam_amd")
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "local_fuser_drive")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_fuser_drive.cpp"),
                                   "-L", libdir, "-lrandt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
            path = os.path.join(tmp, "scans.bin")
            with open(path, "wb") as f:
                f.write(np.array([scans.shape[0], scans.shape[1]], dtype=np.int32).tobytes())
                f.write(np.ascontiguousarray(scans, dtype=np.float32).tobytes())
            best = None
            for rep_ in range(2):
                r = subprocess.run([exe, path, os.path.join(tmp, "p.txt"), "40", "10", "--slam", os.path.join(tmp, "g.txt"), "--timing", "40"],
                                   capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode == 0 and line:
                    j = json.loads(line[-1])
                    if best is None or j["ms_per_scan"] < best["ms_per_scan"]:
                        best = j
            g = open(os.path.join(tmp, "g.txt")).read().splitlines()
            cpp = {"ms_per_scan": best["ms_per_scan"], "scans_per_sec": best["scans_per_sec"], "stream_syncs_per_scan": best["stream_syncs_per_scan"],
                   "device_allocs_per_scan": best["device_allocs_per_scan"], "graph_nodes": sum(1 for ln in g if ln.startswith("node")),
                   "loop_constraints": sum(1 for ln in g if ln.startswith("loop") and ln.endswith(" 1")),
                   "note": "scans 40 .. 299 of the drive (the first submap is the warm-up); the allocator calls are the keyframe scans and finished "
                           "submaps the loop search keeps (scans_ / submaps_ of LocalFuser), not churn"}
    except Exception as e:  # noqa: BLE001
        cpp = {"error": "%s: %s" % (type(e).__name__, e)}
    return {"cpp_facade_drive": cpp, "scans": n_scans, "scans_per_sec": n_scans / el, "ms_per_scan": el / n_scans * 1e3, "graph_nodes": len(s.nodes),
            "loop_constraints": len(loops), "loop_candidates_checked": len(s.loop_log), "pose_graph_optimisations": s.n_optimizations,
            "submaps_finished": s.n_finished_submaps, "loop_closure_ms_total": t_loop * 1e3, "pose_graph_ms_total": t_pg * 1e3,
            "end_pose_error_vs_truth_m": float(np.hypot(est[0] - rel[0], est[1] - rel[1]))}


def polar_odometry(ctx, n_scans):
    """BASELINE config 5, whole loop (side measurement): Oxford-shaped raw polar scans (400 azimuths x 3000 bins,
    19.2 MB each, resident in HBM) -> filterScan -> clustering + NDT -> constant-velocity prediction -> fixed-lag window
    registration -> keyframe merge / submap roll-over, one scan after the other (LocalFuser::processScan call pattern)."""
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import host, odometry, synth

    world = synth.make_world()
    dt = 0.25
    traj = synth.make_trajectory(3300, n_scans, step=0.25)
    dev = torch.device("cuda", ctx.device)
    d_raw = [torch.from_numpy(synth.make_polar_scan(world, traj[i], 61000 + i)).to(dev) for i in range(n_scans)]
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    wp = R.window_params()
    fp = host.filter_params()
    odo = odometry.Odometry(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params()), mp, wp)
    # One untimed pass (kernels, workspaces, first touch of the freshly uploaded scans), then three timed passes over the
    # same drive: this loop keeps the GPU mostly idle between small launches, and the first passes after an idle period run
    # ~1.6x slower than the settled rate (clock ramp); the median pass is reported, all three are listed.
    passes = []
    for rep in range(4):
        odo = odometry.Odometry(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params()), mp, wp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_scans):
            pose = odo.process_scan(d_raw[i], i * dt, polar_filter=fp)
        torch.cuda.synchronize()
        if rep:
            passes.append(time.perf_counter() - t0)
    el = sorted(passes)[1]
    rel = synth.se2_mul3(synth.se2_inv3(traj[0]), traj[-1])
    est = synth.pose4_to_pose3(pose)
    raw_bytes = int(d_raw[0].numel() * 4)
    # the same loop from C++ with the raw scans in HOST memory (tests/cpp/local_fuser_drive.cpp --polar: RadarPreprocessor::processScan
    # through the facade = randt_filter_build, i.e. every scan pays its 19.2 MB PCIe upload): the PCIe-inclusive figure of config 5
    cpp = None
    try:
        import subprocess
        import tempfile

        libdir = os.path.join(ROOT, "randt-slam_amd")
        n_cpp = min(n_scans, 40)
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "local_fuser_drive")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_fuser_drive.cpp"),
                                   "-L", libdir, "-lrandt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
            path = os.path.join(tmp, "polar.bin")
            n_az, n_bins = int(d_raw[0].shape[0]), int(d_raw[0].shape[1])
            with open(path, "wb") as f:
                f.write(np.array([n_cpp, n_az * n_bins], dtype=np.int32).tobytes())
                for i in range(n_cpp):
                    f.write(d_raw[i].cpu().numpy().tobytes())
            r = subprocess.run([exe, path, os.path.join(tmp, "p.txt"), "135", "20", "--polar", str(n_az), str(n_bins), "--timing", "8"],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError("local_fuser_drive --polar: rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
            j = json.loads(line[-1])
            cpp = {"scans": j["scans"], "ms_per_scan": j["ms_per_scan"], "scans_per_sec": j["scans_per_sec"], "raw_GBps_pcie_inclusive": raw_bytes / (j["ms_per_scan"] * 1e-3) / 1e9,
                   "stream_syncs_per_scan": j["stream_syncs_per_scan"], "device_allocs_per_scan": j["device_allocs_per_scan"],
                   "note": "raw polar scans handed over as pageable host buffers, a FRESH 19.2 MB buffer per scan (the runtime pins its pages for every upload: 0.7 .. 1.5 ms; a "
                           "buffer that is reused uploads at 50 GB/s, tools/host_polar_probe.py): upload + filter + clustering + NDT + window registration per scan"}
    except Exception as e:  # noqa: BLE001
        cpp = {"error": "%s: %s" % (type(e).__name__, e)}
    return {"cpp_host_buffers": cpp, "scans": n_scans, "scans_per_sec": n_scans / el, "ms_per_scan": el / n_scans * 1e3, "raw_bytes_per_scan": raw_bytes,
            "raw_GBps": n_scans * raw_bytes / el / 1e9, "pass_ms_per_scan": [p / n_scans * 1e3 for p in passes],
            "registrations": odo.n_registrations, "rejected": odo.n_rejected,
            "end_pose_error_vs_truth_m": float(np.hypot(est[0] - rel[0], est[1] - rel[1]))}


def streaming_odometry(ctx, n_scans, with_cpu):
    """BASELINE config 3 (side measurement, not the headline metric): sequential scans through the
    LocalFuser::processScan call pattern -- scan NDT build, constant-velocity prediction, fixed-lag
    window registration (3 states, motion factors), keyframe merge with insertion delay, submap
    roll-over with overlap -- one scan after the other on one GPU (the path does not shard: scan t
    needs pose t-1).  Inputs resident in HBM; every scan costs one device->host pose read-back."""
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import odometry, synth

    world = synth.make_world()
    dt = 0.25
    traj = synth.make_trajectory(3300, n_scans, step=0.25)
    scans = np.stack([synth.make_scan(world, traj[i], 20000 + i) for i in range(n_scans)])
    d_scans = torch.from_numpy(scans).to(torch.device("cuda", ctx.device))
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    wp = R.window_params()
    odo = odometry.Odometry(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params()), mp, wp)
    for i in range(min(8, n_scans)):                       # warm-up (kernels, workspace)
        odo.process_scan(d_scans[i], i * dt)
    odo = odometry.Odometry(odometry.HipBackend(ctx, R.indoor_map_params(), R.indoor_cluster_params()), mp, wp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    iters = 0
    for i in range(n_scans):
        pose = odo.process_scan(d_scans[i], i * dt)
        iters += int(odo.last_result["iterations"]) if odo.last_result is not None else 0
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    origin_inv = synth.se2_inv3(traj[0])
    rel = synth.se2_mul3(origin_inv, traj[-1])
    est = synth.pose4_to_pose3(pose)
    out = {"scans": n_scans, "scans_per_sec": n_scans / el, "ms_per_scan": el / n_scans * 1e3,
           "mean_lm_iterations_per_scan": iters / max(1, odo.n_registrations), "submaps_finished": odo.n_finished_submaps,
           "end_pose_error_vs_truth_m": float(np.hypot(est[0] - rel[0], est[1] - rel[1]))}
    # BASELINE config 3 asks for "registrations/sec + HBM GB/s": the PMC bytes of the launches one scan costs (committed counter
    # summary; its collection run contains this very loop) x scans/s.  One window is one workgroup on one of 256 compute units
    # walking a dependent chain: the loop moves ~0.6 MB per scan and uses a few GB/s of the 8 TB/s -- latency-bound by construction.
    rows = {"k_ndt_build (one 2000-point scan)": (find_row("k_ndt_build<", 256), 1.0),
            "k_associate (the window's NDT terms)": (find_row("k_associate<false,16", most_dispatched_below=65536), 1.0),
            "k_solve_window": (find_row("k_solve_window<"), 1.0),
            "k_maps_merge (every insertion_step-th scan)": (find_row("k_maps_merge"), 0.25)}
    if all(r is not None for r, _ in rows.values()):
        per_scan = sum(row_bytes(r) * w for r, w in rows.values())
        out["hbm_achieved"] = {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "bytes_per_scan": int(per_scan),
                               "bytes_by_launch": {k: int(row_bytes(r) * w) for k, (r, w) in rows.items()},
                               "achieved": per_scan * n_scans / el / 1e9, "frac": per_scan * n_scans / el / 1e9 / HBM_PEAK_GBS,
                               "note": "FETCH_SIZE x 2 + WRITE_SIZE of the per-scan launches (committed counter summary) x scans/s"}
    else:
        out["hbm_achieved"] = {"frac": None, "counters_refused": "no (current) counter rows for the per-scan launches"}
    if with_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle_backend import OracleBackend

        n_cpu = min(n_scans, 40)
        cpu = odometry.Odometry(OracleBackend(), mp, wp)
        t0 = time.perf_counter()
        for i in range(n_cpu):
            pc = cpu.process_scan(scans[i], i * dt)
        out["cpu_oracle_scans_per_sec"] = n_cpu / (time.perf_counter() - t0)
        out["cpu_oracle_sample"] = "first %d scans, 1 thread (sequential path)" % n_cpu
        # the same drive with the residual blocks of every window problem over all granted cores: what the reference's
        # num_threads = hardware_concurrency() (ndt_matcher.cpp:376) buys on the sequential path (timing only, other summation order)
        import pyoracle as po
        eff, _, _ = effective_cpus()
        cores = max(1, min(po.num_threads(), eff))
        po.set_eval_threads(cores)
        try:
            cpu = odometry.Odometry(OracleBackend(), mp, wp)
            t0 = time.perf_counter()
            for i in range(n_cpu):
                cpu.process_scan(scans[i], i * dt)
            out["cpu_oracle_residual_parallel"] = {"scans_per_sec": n_cpu / (time.perf_counter() - t0), "cores": cores,
                                                   "sample": "the same %d scans, residual blocks over %d OpenMP threads" % (n_cpu, cores)}
        finally:
            po.set_eval_threads(1)
    return out


def config3_replicas(ctx, n_steps, replica_counts=(64, 256, 1024)):
    """BASELINE config 3 does not shard (scan t needs pose t-1: SURVEY 8(e) "replicas only"); its scaling axis is R independent
    odometry loops on one GPU.  randt-slam_amd/odometry.py::ReplicaOdometry advances R of them in lock-step -- per step ONE NDT
    build launch (R scans), ONE randt_register_window_batch (R windows, a workgroup each) and, on keyframe steps, ONE
    randt_maps_merge_batch -- where R Odometry objects need R contexts / streams and a host round trip each.  Replica r
    replays config 3's drive from scan r on (every replica sees other scans at every step).  Reported per R: scans/s of the
    whole loop (Python harness: the per-replica host work -- constant-velocity prediction, state packing -- is in it), the
    window call's share, and the window kernel's issue-slot fraction of the CHIP from the committed counter row of
    k_solve_window (one window alone: 0.26 of ONE compute unit's issue rate = 0.001 of the chip)."""
    import torch

    import randt_slam_amd as R
    from randt_slam_amd import host, odometry, synth

    rmax = max(replica_counts)
    world = synth.make_world()
    dt = 0.25
    traj = synth.make_trajectory(3300, n_steps + rmax, step=0.25)
    scans = np.stack([synth.make_scan(world, traj[i], 20000 + i) for i in range(n_steps + rmax)])
    d_all = torch.from_numpy(scans).to(torch.device("cuda", ctx.device))
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    wp = R.window_params()
    st = torch.cuda.current_stream()
    out = {"workload": "R replicas of config 3's loop in lock-step, replica r = the drive from scan r on; %d steps per replica, one submap roll-over" % n_steps,
           "single_loop_reference": "config3_streaming_odometry (one Odometry object, one window per launch)"}
    cyc = WINDOW_ROW.get("valu_issue_cycles")
    real_call = host.register_window_batch
    for n_rep in replica_counts:
        acc = {"host_s": 0.0, "ev": []}

        def timed_call(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            t0 = time.perf_counter()
            r = real_call(*a, **k)
            acc["host_s"] += time.perf_counter() - t0
            e1.record(st)
            acc["ev"].append((e0, e1))
            return r

        for timed in (False, True):
            rep = odometry.ReplicaOdometry(ctx, n_rep, R.indoor_map_params(), R.indoor_cluster_params(), mp, wp)
            host.register_window_batch = timed_call if timed else real_call
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n_steps if timed else min(12, n_steps)):
                    poses = rep.process_scans(d_all[i:i + n_rep], i * dt)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
            finally:
                host.register_window_batch = real_call
        dev_ms = float(np.mean([a.elapsed_time(b) for a, b in acc["ev"]]))
        origin_inv = synth.se2_inv3(traj[0])
        est = synth.pose4_to_pose3(poses[0])
        rel = synth.se2_mul3(origin_inv, traj[n_steps - 1])
        sect = {"replicas": n_rep, "steps": n_steps, "scans_per_sec": n_rep * n_steps / el, "ms_per_step": el / n_steps * 1e3,
                "window_batch_call_ms_per_step": acc["host_s"] / max(1, len(acc["ev"])) * 1e3, "window_batch_device_ms": dev_ms,
                "windows_per_sec_in_the_window_call": n_rep / (acc["host_s"] / max(1, len(acc["ev"]))),
                "registrations": rep.n_registrations, "rejected": rep.n_rejected, "submaps_finished": rep.n_finished_submaps,
                "replica0_end_pose_error_vs_truth_m": float(np.hypot(est[0] - rel[0], est[1] - rel[1]))}
        if cyc:
            sect["window_kernel_issue_frac_of_chip"] = n_rep * float(cyc) / (dev_ms * 1e-3) / (VALU_PEAK * 1e9)
            sect["window_kernel_issue_cycles_per_window"] = float(cyc)
        out["R%d" % n_rep] = sect
        del rep
    return out


def cpp_local_fuser_drive(ctx, n_scans, python_ms_per_scan=None):
    """The drop-in path as the reference's node would run it (round-4 verdict, item 1): a C++ caller of include/randt_facade.hpp
    with LocalFuser::processScan's call pattern (tests/cpp/local_fuser_drive.cpp: Maps BY VALUE -- every copy the reference makes,
    local_fuser.cpp:128-136,173-178 --, the reference-signature Matcher::estimateTransformCeres, transformMap + mergeMapCell), fed
    HOST buffers scan by scan.  Same synthetic drive as config 3.  Reported: wall time per scan after a warm-up, and what the
    context's storage pool / pinned ring leave of the allocator: hipMalloc / hipFree / stream synchronisations per steady-state
    scan (randt_ctx_pool_stats).  Four legs: packed x y z I points through Map::addScan, pcl::PointXYZI records (32 B, the
    reference's own host layout) through Map::addScan, the reference's own insertion -- host clustering (Grid::cluster +
    labelClouds) + HierarchicalMap::addClusters on the cluster list (ndt_hierarchical_map.cpp:28-33; one launch since round 5) --
    and that loop spelled out as one Map::insertCluster call per cluster."""
    import subprocess
    import tempfile

    from randt_slam_amd import synth

    world = synth.make_world()
    traj = synth.make_trajectory(3300, n_scans, step=0.25)
    scans = np.ascontiguousarray(np.stack([synth.make_scan(world, traj[i], 20000 + i) for i in range(n_scans)]), dtype=np.float32)
    libdir = os.path.join(ROOT, "randt-slam_amd")
    out = {"workload": "config 3's drive (%d sequential 2000-point scans, indoor parameters, 135-state submaps with 20-state overlap) from HOST "
                       "buffers through the C++ facade, Maps by value" % n_scans}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "local_fuser_drive")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "local_fuser_drive.cpp"),
                               "-L", libdir, "-lrandt_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
        path = os.path.join(tmp, "scans.bin")
        with open(path, "wb") as f:
            f.write(np.array([scans.shape[0], scans.shape[1]], dtype=np.int32).tobytes())
            f.write(scans.tobytes())
        # steady state = behind the first submap roll-over (scan 135) and its 20-scan overlap: by then the pool has seen every
        # size the drive asks for and the workspaces have their final size
        warm = 160 if n_scans >= 300 else n_scans // 4
        poses = {}
        for key, flags, n in (("add_scan_packed", [], n_scans), ("add_scan_pointxyzi", ["--xyzi8"], n_scans),
                              ("add_clusters_pointxyzi", ["--xyzi8", "--clusters"], n_scans),
                              ("insert_cluster_loop_pointxyzi", ["--xyzi8", "--cluster-loop"], min(n_scans, 120))):
            if n < n_scans:   # a shorter drive: the same file header with fewer scans
                sub = os.path.join(tmp, "scans_%d.bin" % n)
                with open(sub, "wb") as f:
                    f.write(np.array([n, scans.shape[1]], dtype=np.int32).tobytes())
                    f.write(scans[:n].tobytes())
            else:
                sub = path
            pf = os.path.join(tmp, key + ".txt")
            best = None
            for rep in range(2):   # the first pass after an idle period runs slower (clock ramp): the better of two
                r = subprocess.run([exe, sub, pf, "135", "20", "--timing", str(warm if n == n_scans else n // 4)] + flags, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("local_fuser_drive %s: rc %d: %s" % (key, r.returncode, (r.stdout + r.stderr)[-400:]))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
                j = json.loads(line)
                if best is None or j["ms_per_scan"] < best["ms_per_scan"]:
                    best = j
            out[key] = best
            poses[key] = np.loadtxt(pf)
        out["poses_equal_across_legs"] = {
            "packed_vs_pointxyzi_max_abs": float(np.abs(poses["add_scan_packed"] - poses["add_scan_pointxyzi"]).max()),
            "add_scan_vs_add_clusters_max_abs": float(np.abs(poses["add_scan_pointxyzi"] - poses["add_clusters_pointxyzi"]).max()),
            "add_scan_vs_insert_cluster_loop_max_abs": float(np.abs(poses["add_scan_pointxyzi"][:len(poses["insert_cluster_loop_pointxyzi"])] - poses["insert_cluster_loop_pointxyzi"]).max())}
    if python_ms_per_scan:
        out["python_resident_loop_ms_per_scan"] = python_ms_per_scan
        out["cpp_over_python_resident"] = out["add_scan_pointxyzi"]["ms_per_scan"] / python_ms_per_scan
    return out


def cpu_baseline(prob, mp, gpu_pose, budget_s):
    """The CPU oracle (a restatement 'port', not Ceres) on the box's host cores, OpenMP over
    registrations, on a bounded sample of the SAME batch; also yields the pose error GPU-vs-oracle."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as po
    from randt_slam_amd import synth

    ip = synth.indoor_params()
    fixed = []
    for sm in prob["submaps"]:
        sub = po.Map(ip["size_x"], ip["size_y"], ip["resolution"], (0, 0), ip["max_neighbour_dist"], ip["min_points_per_cell"])
        for t in range(len(sm["kf_scans"])):
            s = po.Map(ip["size_x"], ip["size_y"], ip["resolution"], (0, 0), ip["max_neighbour_dist"], ip["min_points_per_cell"], 512)
            s.build(sm["kf_scans"][t], ip["n_clusters"], ip["max_range"])
            s.transform(synth.pose3_to_pose4(sm["kf_rel"][t]))
            sub.merge(s)
        fixed.append(sub)
    op = po.default_params()
    for name, _ in mp._fields_:
        if name != "reserved":
            setattr(op, name, getattr(mp, name))
    g4 = synth.pose3_to_pose4(prob["guess"])
    eff, logical, quota = effective_cpus()
    cores = max(1, min(po.num_threads(), eff))     # one OpenMP thread per CPU the cgroup really grants
    B = len(prob["scans"])
    done, t_total, poses = 0, 0.0, None
    while t_total < budget_s:
        t0 = time.perf_counter()
        fail, poses, cost, iters = po.register_batch(prob["scans"], fixed, prob["submap_of"], op, g4, ip["n_clusters"],
                                                     ip["max_range"], n_threads=cores)
        t_total += time.perf_counter() - t0
        done += B
    # single-thread leg: the first 64 registrations of the batch, repeated until the budget is spent
    n1, done1, t1 = min(B, 64), 0, 0.0
    while t1 < budget_s:
        t0 = time.perf_counter()
        po.register_batch(prob["scans"][:n1], fixed, prob["submap_of"][:n1], op, g4[:n1], ip["n_clusters"], ip["max_range"], n_threads=1)
        t1 += time.perf_counter() - t0
        done1 += n1
    err_t = float(np.abs(gpu_pose[:, 2:] - poses[:, 2:]).max())
    dth = np.arctan2(gpu_pose[:, 1], gpu_pose[:, 0]) - np.arctan2(poses[:, 1], poses[:, 0])
    err_r = float(np.abs((dth + np.pi) % (2 * np.pi) - np.pi).max())
    return {
        "cpu_baseline": {
            "value": done / t_total, "unit": "registrations/s", "cores": cores, "kind": "port",
            "host_logical_cpus": logical, "cgroup_cpu_quota": quota,
            "sample": "%d passes of the same 512-registration batch through the OpenMP CPU oracle (%.1f s wall, %d threads = the CPUs "
                      "the container's cgroup quota grants; the host shows %d logical CPUs)" % (done // B, t_total, cores, logical),
            "single_thread": {"value": done1 / t1, "unit": "registrations/s", "cores": 1,
                              "sample": "%d passes of the batch's first %d registrations, 1 thread (%.1f s wall)" % (done1 // n1, n1, t1)},
        },
        "pose_err_vs_oracle": {"max_abs_translation_m": err_t, "max_abs_rotation_rad": err_r, "tolerance": [1e-4, 1e-4]},
    }


if __name__ == "__main__":
    main()
    if _HUNG_THREADS:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
