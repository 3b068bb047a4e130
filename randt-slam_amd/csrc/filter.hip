// Radar scan filter for gfx950 -- SURVEY row f-1, the HBM-streaming stage in front of the NDT build
// (compiled with -ffp-contract=off: the emitted points must equal the reference's bit for bit).
//
// Replaces RadarPreprocessor::filterScan (src/radar_preprocessing/radar_preprocessor.cpp:45-125):
// per azimuth the strongest return inside (min_range, max_range), then the run of monotonically
// decreasing intensity around it, thresholded by min_intensity, transformed sensor -> base.
//
//   k_filter_rows   one 256-thread WORKGROUP per azimuth row (round 5; rounds 3 / 4: history below).  Per row:
//                   1. the row of the raw polar scan (16 B / point, 19.2 MB for 400 x 3000) is read exactly once with
//                      coalesced dwordx4 loads, twelve per lane = the whole row in flight at once; the arg-max (strict '>',
//                      first index wins) stays in registers, is combined by shuffles and, over the four wavefronts, through
//                      LDS behind ONE barrier; the same pass checks that the cloud really is organised azimuth after azimuth
//                      (the reference detects azimuth changes with |atan2 - current| > 1e-4 while walking the cloud
//                      sequentially): a cross / dot test flags, a flagged row is walked again with the exact atan2f;
//                   2. the row's detection is expanded towards / away from the sensor by wavefront 0 while the
//                      row is cache-hot (expand_both below); the same loads count the run's points that pass the output
//                      thresholds and -- for runs of <= FILT_STAGE kept points that end within 32 bins on both sides:
//                      nearly all -- produce the output points themselves (the "stage"); a 32-byte row record.
//   k_filter_emit   one workgroup per scan: replays the reference's detection-list semantics (last azimuth never
//                   flushed, the very first boundary pushes index 0), block-scans the kept counts over the rows and
//                   emits the points and the per-azimuth peaks in the reference's order: staged rows are copied (record
//                   and stage arrive in one round trip), the others re-read their run, eight independent loads at a time.
// Measured (16 scans per launch, 307 MB, rocprofv3 averages; a bare read of the same bytes takes 44 .. 45 us when consecutive
// launches meet their lines in the 256 MB Infinity Cache and 48.4 .. 49.5 us per 307 MB of a 1.2 GB buffer, i.e. from HBM:
// tools/hbm_stream_probe.hip; 51.5 us as launches of 16 scans over distinct inputs):
//   rounds 3 / early 4  a PERSISTENT workgroup walking rows, barrier between arg-max and expansion: 58.2 + 7.6 (emission) us; with
//                       expansion and per-point tests compiled out still 53.6: it paid for the barrier, behind which four wavefronts
//                       have nothing in flight; next row in a second register set (191 registers, two per CU) 93;
//                       non-temporal row loads 100; 96 / 80 registers (spills) 84 / 104; emission behind a ticket per row 130;
//                       next row's loads issued before the barrier (+ a fifth wavefront for the expansion) 54 .. 69
//   round 4             wavefront per row 54.8 -> ring of loads 53.2 -> exact test out of the loop, scalar row base, one
//                       dwordx4 per point 51.4 over one input, 56.3 .. 56.6 over distinct inputs; emission 7.6 -> 5.6 us with the
//                       stage.  ONE scan per launch: 11.97 + 5.22 us = 0.14 of 8 TB/s (400 wavefronts, 47 dependent rounds each)
//   round 5 (this file) a workgroup per ROW (not persistent: three wavefronts retire at the barrier, the dispatcher refills):
//                       52.6 + 5.6 us over distinct inputs, ONE scan 7.9 + 4.4 us (profiles/experiments/r05_filter_workgroup_per_row.md;
//                       the emission folded into the row kernel behind a per-scan ticket: +12 .. +290 us, priced there)
#include "randt_internal.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

#ifndef FILT_BLOCK
#define FILT_BLOCK 256
#endif
#define FILT_WAVES (FILT_BLOCK / 64)
#define FILT_STAGE 4     // kept points per row that the row kernel hands to the emission ready-made (2 float4 each)
#define FILT_EBLOCK 512  // emission kernel: all azimuth rows of a 400-row scan in one round
#ifndef FILT_UNROLL
#define FILT_UNROLL 12
#endif
// loads in flight per lane: rows of up to 12 * 256 = 3072 bins are fetched in one go

namespace {

// std::hypot(float, float) as glibc evaluates it: double sqrt, one rounding.
__device__ __forceinline__ float hypot_f(float x, float y) { return (float)sqrt((double)x * (double)x + (double)y * (double)y); }

// what the row workgroups leave for the emitting workgroup (32 bytes)
struct RowRec {
  int32_t m;        // cloud index of the row's detection, -1: none
  int32_t closer;   // first / last cloud index of the expanded run
  int32_t further;
  int32_t kept;     // points of the run that pass the range / intensity thresholds
  float angle;      // atan2 of the row's first point (the reference's current_angle)
  float maxi;       // peak intensity
  float peak_range; // hypot of the detection (the emission's per-azimuth peak record)
  int32_t bad;      // bit 0: an azimuth change inside the row (the scan is not organised azimuth after azimuth);
                    // bit 1: all of the row's kept points are in the stage
};

struct FilterArgs {
  const float* raw;   // [n_scans][n_az][n_bins][stride]
  int n_scans, n_az, n_bins, stride, ioff;
  float min_d, max_d, min_i, thr;
  double lo2, hi2;    // range test on the squared distance: min_d < hypot(x, y) < max_d  <=>  lo2 <= x^2 + y^2 <= hi2
  float T[12];
  float* out_pts;     // [n_scans][pitch_out][4]
  float* out_polar;   // nullable [n_scans][pitch_out][2]
  float* peaks;       // nullable [n_scans][n_az][3]
  int32_t* out_counts;
  int32_t* peak_counts;  // nullable
  int32_t* status;       // [n_scans] 0 ok, 1 not azimuth-organised, 2 output overflow
  int pitch_out;
  int out_vec;        // out_pts is 16-byte aligned
  // scratch
  RowRec* rows;       // [n_scans][n_az]
  float4* stage;      // [n_scans][n_az][FILT_STAGE][2]: {x' y' z' I}, {atan2 range - -} of a row's first kept points
  // SRC_RASTER only: the scan as an azimuth x range intensity raster and its two tables (raw is null then)
  const unsigned char* raster;  // [n_scans] scan_pitch bytes, rows of row_pitch bytes (16-byte aligned, pitch % 16 == 0)
  const float* cossin;          // [n_scans][n_az][2]
  const float* ranges;          // [n_bins]
  long long row_pitch, scan_pitch;
  float iscale;
  int elem;                     // RANDT_RASTER_U8 / U16 / F32
  int rng_vec;                  // ranges is 16-byte aligned
};

// Where a kernel finds the points of a scan.  SRC_PACKED: 16-byte x y z I records (one dwordx4 load per point), known at
// compile time so that a row's loads are issued back to back with no branch between them; SRC_STRIDED: records of A.stride
// floats; SRC_RASTER: one intensity per bin, the point is formed from the tables -- x = ranges[b] * c_a, y = ranges[b] * s_a,
// z = 0, I = (float)v * iscale, one fp32 multiply each: what a converter would have written into the packed cloud.
enum { SRC_STRIDED = 0, SRC_PACKED = 1, SRC_RASTER = 2 };
struct ScanSrc {
  const float* base;          // cloud sources: the scan's first record
  const unsigned char* ras;   // SRC_RASTER: the scan's first row
  const float* cs;            //             the scan's (cos, sin) per azimuth
};
template <int SRC>
__device__ __forceinline__ ScanSrc scan_src(const FilterArgs& A, int scan) {
  ScanSrc S;
  S.base = SRC == SRC_RASTER ? nullptr : A.raw + (size_t)scan * A.n_az * A.n_bins * A.stride;
  S.ras = SRC == SRC_RASTER ? A.raster + (size_t)scan * A.scan_pitch : nullptr;
  S.cs = SRC == SRC_RASTER ? A.cossin + (size_t)scan * A.n_az * 2 : nullptr;
  return S;
}

// point i (cloud index within the scan, < 2^30) of a scan
template <int SRC>
__device__ __forceinline__ void fetch(const FilterArgs& A, const ScanSrc& S, long long i, float& x, float& y, float& in) {
  if (SRC == SRC_PACKED) {
    const float4 p = reinterpret_cast<const float4*>(S.base)[i];
    x = p.x;
    y = p.y;
    in = A.ioff == 3 ? p.w : (A.ioff == 2 ? p.z : (A.ioff == 1 ? p.y : p.x));
  } else if (SRC == SRC_RASTER) {
    const unsigned a = (unsigned)i / (unsigned)A.n_bins, b = (unsigned)i - a * (unsigned)A.n_bins;
    const float r = A.ranges[b];
    x = r * S.cs[2 * a];
    y = r * S.cs[2 * a + 1];
    const unsigned char* row = S.ras + (size_t)a * A.row_pitch;
    const float v = A.elem == RANDT_RASTER_U8 ? (float)row[b]
                                              : (A.elem == RANDT_RASTER_U16 ? (float)reinterpret_cast<const unsigned short*>(row)[b]
                                                                            : reinterpret_cast<const float*>(row)[b]);
    in = v * A.iscale;
  } else {
    const float* p = S.base + (size_t)i * A.stride;
    x = p[0];
    y = p[1];
    in = p[A.ioff];
  }
}

__device__ __forceinline__ bool keep_point(const FilterArgs& A, float x, float y, float in, float& dist) {
  dist = hypot_f(x, y);
  return (double)dist > (double)A.min_d && (double)dist < (double)A.max_d && (double)in > (double)A.min_i;
}

template <int NW>
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* scratch, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const unsigned long long s = scratch[w];
    if (w < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

// the output point of a kept return: pcl::transformPointCloud with initial_transform_radar_baselink_ (:124)
__device__ __forceinline__ float4 to_base(const FilterArgs& A, float x, float y, float z, float in) {
  float4 o;
  o.x = ((A.T[0] * x + A.T[1] * y) + A.T[2] * z) + A.T[3];
  o.y = ((A.T[4] * x + A.T[5] * y) + A.T[6] * z) + A.T[7];
  o.z = ((A.T[8] * x + A.T[9] * y) + A.T[10] * z) + A.T[11];
  o.w = in;
  return o;
}
template <int SRC>
__device__ __forceinline__ float fetch_z(const FilterArgs& A, const ScanSrc& S, long long i) {
  if (SRC == SRC_RASTER) return 0.f;
  return SRC == SRC_PACKED ? reinterpret_cast<const float4*>(S.base)[i].z : (A.stride > 2 ? S.base[(size_t)i * A.stride + 2] : 0.f);
}
template <int SRC>
__global__ __launch_bounds__(FILT_EBLOCK) void k_filter_emit(FilterArgs A) {
  __shared__ unsigned long long scratch[FILT_EBLOCK / 64];
  const int scan = blockIdx.x, tid = threadIdx.x;
  const ScanSrc S = scan_src<SRC>(A, scan);
  const RowRec* rows = A.rows + (size_t)scan * A.n_az;
  int bad = 0;
  int n_det = 0, n_out = 0;
  float* out = A.out_pts + (size_t)scan * A.pitch_out * 4;
  float* pol = A.out_polar ? A.out_polar + (size_t)scan * A.pitch_out * 2 : nullptr;
  float* pk = A.peaks ? A.peaks + (size_t)scan * A.n_az * 3 : nullptr;
  // the last azimuth is never flushed (the push happens when the NEXT azimuth starts): its record says "none"
  const int n_rows = A.n_az - 1;
  for (int r0 = 0; r0 < A.n_az; r0 += FILT_EBLOCK) {
    const int r = r0 + tid;
    RowRec rec;
    rec.m = -1;
    rec.closer = 0;
    rec.further = -1;
    rec.kept = 0;
    rec.angle = rec.maxi = rec.peak_range = 0.f;
    rec.bad = 0;
    float4 st[2 * FILT_STAGE];  // the row's staged points, fetched in the same round trip as its record
#pragma unroll
    for (int k = 0; k < 2 * FILT_STAGE; ++k) st[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < n_rows) {
      rec = rows[r];
      const float4* sp = A.stage + ((size_t)scan * A.n_az + r) * (2 * FILT_STAGE);
#pragma unroll
      for (int k = 0; k < 2 * FILT_STAGE; ++k)
        if (pol || !(k & 1)) st[k] = sp[k];
    }
    // (the same round trip serves the organisation check: an azimuth change inside a row -- k_filter_rows --, and consecutive
    // azimuths must differ by more than the reference's 1e-4 rad threshold; the last row's record only takes part here)
    if (r < A.n_az) {
      const RowRec cur = r < n_rows ? rec : rows[r];
      if (cur.bad & 1) bad = 1;
      if (r > 0 && !(fabsf(cur.angle - rows[r - 1].angle) > 0.0001)) bad = 1;
    }
    const bool det = rec.m >= 0;
    // ONE block scan for both running counts: detections in the upper, kept points in the lower 32 bits (neither can carry:
    // a scan holds < 2^30 points)
    unsigned long long tot;
    const unsigned long long at = block_excl_scan<FILT_EBLOCK / 64>(det ? ((1ull << 32) | (unsigned long long)(unsigned)rec.kept) : 0ull, scratch, &tot);
    const int tot_det = (int)(tot >> 32), tot_kept = (int)(unsigned)tot;
    const int det_at = n_det + (int)(at >> 32);
    int out_at = n_out + (int)(unsigned)at;
    if (det) {
      if (pk) {
        pk[3 * det_at + 0] = rec.angle;
        pk[3 * det_at + 1] = rec.peak_range;
        pk[3 * det_at + 2] = rec.maxi;
      }
      auto put = [&](const float4& o, float ang, float dist) {
        if (out_at < A.pitch_out) {
          if (A.out_vec) {  // 16-byte aligned output: one store per point
            reinterpret_cast<float4*>(out)[out_at] = o;
          } else {
            float* op = out + (size_t)out_at * 4;
            op[0] = o.x, op[1] = o.y, op[2] = o.z, op[3] = o.w;
          }
          if (pol) {
            pol[2 * (size_t)out_at + 0] = ang;
            pol[2 * (size_t)out_at + 1] = dist;
          }
        }
        ++out_at;
      };
      if (rec.bad & 2) {
        // the row kernel left the run's kept points ready-made
#pragma unroll
        for (int k = 0; k < FILT_STAGE; ++k)
          if (k < rec.kept) put(st[2 * k], st[2 * k + 1].x, st[2 * k + 1].y);
      } else {
        // the run, eight bins per round trip (the loads of a round are independent; the stores are not)
        for (long long j0 = rec.closer; j0 <= rec.further; j0 += 8) {
          float x[8], y[8], in[8], z[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const long long j = j0 + u;
            x[u] = y[u] = in[u] = z[u] = 0.f;
            if (j <= rec.further) {
              fetch<SRC>(A, S, j, x[u], y[u], in[u]);
              z[u] = fetch_z<SRC>(A, S, j);
            }
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            float dist;
            if (j0 + u <= rec.further && keep_point(A, x[u], y[u], in[u], dist)) put(to_base(A, x[u], y[u], z[u], in[u]), pol ? atan2f(y[u], x[u]) : 0.f, dist);
          }
        }
      }
    }
    n_det += tot_det;
    n_out += tot_kept;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    A.out_counts[scan] = n_out <= A.pitch_out ? n_out : A.pitch_out;
    if (A.peak_counts) A.peak_counts[scan] = n_det;
    A.status[scan] = n_out > A.pitch_out ? 2 : (bad ? 1 : 0);  // written, not max-ed: no clearing launch in front of the two kernels
  }
}

// The run expansion (:80-108) in direction DIR = -1 (towards the sensor) / +1 (away from it): the first d >= 0 at which
//   (m + DIR (d + 1) leaves the cloud)  or  hypot(a) - hypot(b) > thr  or  I(a) <= I(b)  or  hypot(a) < min_range
// with a = m + DIR d, b = a + DIR; the run ends at that a.  Sequential in the reference; here both directions in ONE
// wavefront: lanes 0..31 walk inwards, lanes 32..63 outwards, 32 values of d per step and direction, one lane per bin
// evaluates the stopping rule and the lowest stopping lane of a half ends its walk (lanes beyond it evaluate bins the
// reference never touches: discarded); the loads of both directions share a round trip (runs are a handful of bins: 2
// kept points per azimuth in the Oxford-shaped scans).
// kept: how many bins of the walked parts (d = 0 .. stop inwards, d = 1 .. stop outwards, so that the detection itself
// is counted once) pass the output thresholds (:110-118) -- the same loads serve both questions.
template <int SRC>
__device__ __forceinline__ bool expand_both(const FilterArgs& A, const ScanSrc& S, long long n, long long m, int lane, long long& closer, long long& further,
                                            int& kept, float& range_m, float4* stage) {
  const int half = lane >> 5, l = lane & 31;
  const long long dir = half ? 1 : -1;
  bool done_c = false, done_f = false, staged = false;
  closer = further = m;
  kept = 0;
  range_m = 0.f;
  for (long long d0 = 0; !(done_c && done_f); d0 += 32) {
    const long long a = m + dir * (d0 + l), b = a + dir;
    const bool live = half ? !done_f : !done_c;
    const bool a_in = live && a >= 0 && a <= n - 1, b_in = b >= 0 && b <= n - 1;
    bool stop = true, keep = false;
    float ha = 0.f, ax = 0.f, ay = 0.f, ai = 0.f;
    if (a_in) {
      float bx = 0.f, by = 0.f, bi = 0.f;
      fetch<SRC>(A, S, a, ax, ay, ai);
      if (b_in) fetch<SRC>(A, S, b, bx, by, bi);
      keep = keep_point(A, ax, ay, ai, ha) && (half == 0 || d0 + l > 0);  // the detection itself is counted once (inward half)
      if (b_in) stop = ((double)(ha - hypot_f(bx, by)) > (double)A.thr) || (ai <= bi) || ((double)ha < (double)A.min_d);
    }
    if (d0 == 0) range_m = __shfl(ha, 0, 64);  // hypot of the detection: the per-azimuth peak record
    const unsigned long long mask = __ballot(stop), kmask = __ballot(keep);
    const unsigned int mc = (unsigned int)mask, mf = (unsigned int)(mask >> 32), kc = (unsigned int)kmask, kf = (unsigned int)(kmask >> 32);
    unsigned int vc = 0, vf = 0;  // the kept bins of this step that belong to the run
    if (!done_c) {
      if (mc) {
        const int first = __ffs((int)mc) - 1;
        vc = kc & (first == 31 ? ~0u : ((1u << (first + 1)) - 1u));
        closer = m - (d0 + first);
        done_c = true;
      } else {
        vc = kc;
      }
    }
    if (!done_f) {
      if (mf) {
        const int first = __ffs((int)mf) - 1;
        vf = kf & (first == 31 ? ~0u : ((1u << (first + 1)) - 1u));
        further = m + (d0 + first);
        done_f = true;
      } else {
        vf = kf;
      }
    }
    kept += __popc(vc) + __popc(vf);
    // A run that ends within the first step on both sides (nearly all do) and keeps <= FILT_STAGE points hands them to the
    // emission ready-made, in cloud order (inward lanes: higher lane = lower index): the emission then has no second,
    // dependent look at the raw scan.  Same expressions as the emission's own path (to_base, atan2f, keep_point's range).
    if (d0 == 0 && done_c && done_f && stage && kept <= FILT_STAGE) {
      staged = true;
      const bool mine = half ? ((vf >> l) & 1u) : ((vc >> l) & 1u);
      if (mine) {
        const int rank = half ? __popc(vc) + __popc(vf & ((1u << l) - 1u)) : __popc(l == 31 ? 0u : (vc >> (l + 1)));
        stage[2 * rank] = to_base(A, ax, ay, fetch_z<SRC>(A, S, a), ai);
        if (A.out_polar) stage[2 * rank + 1] = make_float4(atan2f(ay, ax), ha, 0.f, 0.f);
      }
    }
  }
  return staged;
}

// The per-point steps of a row kernel, shared by the cloud and the raster row kernels.  The kernels must stay on the HBM
// roofline, so the two per-point tests are restated without transcendental work: (a) range: hypot() in float after a double
// sqrt is monotone in d2 = x^2 + y^2, so the launcher bisects the two double thresholds once; (b) organisation: a point whose
// direction is within 4e-5 rad of the row's first point (|cross| <= 4e-5 dot, dot > 0) cannot differ from it by 1e-4 in atan2f;
// only other points (none in an organised scan) and rows next to the +-pi cut take the exact atan2f comparison (exact_change).
struct RowWalk {
  float x0, y0;        // the row's first point: its angle is the reference's current_angle for this azimuth
  float best_i;        // max_intensity starts at 0: only intensity > 0 can win
  int best_idx;
  bool suspect;
  __device__ __forceinline__ RowWalk(float x, float y) : x0(x), y0(y), best_i(0.f), best_idx(0x7fffffff), suspect(false) {}
  // |atan2f(y0, x0)| >= 3.14, decided without the atan2f (a superset: tan(pi - 3.14) = 0.00159)
  __device__ __forceinline__ bool near_cut() const { return x0 < 0.f && fabsf(y0) <= 0.002f * fabsf(x0); }
  // (dot > 0: a zero-filled return passes 0 <= 0, but the reference's atan2(0, 0) = 0 starts a new azimuth there)
  __device__ __forceinline__ bool off_direction(float px, float py) const {
    const float cross = x0 * py - y0 * px, dot = x0 * px + y0 * py;
    return !(fabsf(cross) <= 4e-5f * dot) || !(dot > 0.f);
  }
  __device__ __forceinline__ void visit(const FilterArgs& A, int b, float px, float py, float pin) {
    suspect |= off_direction(px, py);
    const double d2 = (double)px * (double)px + (double)py * (double)py;
    if (d2 >= A.lo2 && d2 <= A.hi2) {
      if (pin > best_i) {  // a lane meets its bins in increasing order: strict '>' keeps the first
        best_i = pin;
        best_idx = b;
      }
    }
  }
  // arg-max over the wavefront: larger intensity wins, ties -> smaller index (strict '>', first index wins)
  __device__ __forceinline__ void reduce_wave() {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oi = __shfl_xor(best_i, off, 64);
      const int ox = __shfl_xor(best_idx, off, 64);
      if (oi > best_i || (oi == best_i && ox < best_idx)) {
        best_i = oi;
        best_idx = ox;
      }
    }
  }
  // the exact organisation test of one point of a flagged row (a0 = atan2f(y0, x0), cut = !(|a0| < 3.14)): an azimuth change
  // inside the row as the reference sees it
  __device__ __forceinline__ bool exact_change(float a0, bool cut, float px, float py) const {
    return (cut || off_direction(px, py)) && fabsf(atan2f(py, px) - a0) > 0.0001;
  }
};

// What one wavefront does with its row's arg-max: the detection (with the reference's quirks), the run around it and the
// 32-byte row record.  Shared by the cloud and the raster row kernels.
template <int SRC>
__device__ __forceinline__ void finish_row(const FilterArgs& A, const ScanSrc& S, long long g, int row, float best_i, int best_idx, float a0, int bad, int lane) {
  const long long n = (long long)A.n_az * A.n_bins, r0 = (long long)row * A.n_bins;
  // the row's detection; quirk: the first boundary pushes current_max_idx = 0 even if azimuth 0 had no valid return;
  // the last azimuth is never flushed
  long long m = (best_i > 0.f && best_idx != 0x7fffffff) ? r0 + best_idx : -1;
  float pk_i = best_i;
  if (row == 0 && m < 0) {
    m = 0;
    pk_i = 0.f;
  }
  if (row == A.n_az - 1) m = -1;
  long long closer = 0, further = -1;
  int kept = 0;
  float range_m = 0.f;
  bool staged = false;
  if (m >= 0) staged = expand_both<SRC>(A, S, n, m, lane, closer, further, kept, range_m, A.stage + (size_t)g * (2 * FILT_STAGE));  // uniform over the wavefront
  if (lane == 0) {
    RowRec rec;
    rec.m = (int32_t)m;
    rec.closer = (int32_t)closer;
    rec.further = (int32_t)further;
    rec.kept = kept;
    rec.angle = a0;
    rec.maxi = pk_i;
    rec.peak_range = range_m;
    rec.bad = (bad ? 1 : 0) | (staged ? 2 : 0);
    A.rows[g] = rec;
  }
}

// One 256-thread WORKGROUP per azimuth row (round 5).  The whole row -- up to FILT_UNROLL x 256 = 3072 bins, 48 KB -- is in
// flight at once, twelve dwordx4 loads per lane issued back to back; every lane keeps the arg-max of its own bins, a wavefront
// reduces with shuffles, the four partial results meet in LDS behind ONE barrier, and wavefront 0 alone expands the run while
// the row is cache-hot (expand_both) and writes the row record; the other three retire at the barrier.
// Why not the wavefront-per-row kernel of round 4 any more (history at the top of the file): a launch of ONE scan has 400 rows
// = 400 wavefronts for 1024 SIMDs, each walking its row through a ring of twelve loads -- 47 dependent rounds, 12 us, 0.14 of
// the HBM rate (round-4 verdict).  Split four ways the row needs ONE round trip, and tools/filter_ticket_probe.hip measured the
// organisation ahead at every launch size: 6.8 against 9.7 us per scan launched alone, 50.5 against 60.8 us per 16 scans over
// distinct inputs (a bare 16-scan read: 51.5).  The same probe priced the remaining idea -- folding the emission into the scan's
// last-arriving workgroup behind a device-scope ticket -- at +70 .. +290 us per 16 scans (one __threadfence per workgroup walks
// the L2): the emission stays a launch of its own.
#ifndef FILT_WPE
#define FILT_WPE 4
#endif
#define FILT_OCC __attribute__((amdgpu_waves_per_eu(FILT_WPE, FILT_WPE)))
// I3: the intensity is the fourth float of a packed record (x y z I, the reference's PointXYZI) -- known at compile time so
// that the visiting code has no branch on ioff
template <bool PACKED, bool I3>
__global__ __launch_bounds__(FILT_BLOCK) FILT_OCC void k_filter_rows(FilterArgs A) {
  __shared__ float s_best[FILT_WAVES];
  __shared__ int s_idx[FILT_WAVES], s_flag[FILT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long g = blockIdx.x;  // scan * n_az + row
  const int scan = (int)(g / A.n_az), row = (int)(g - (long long)scan * A.n_az);
  const float* base = A.raw + (size_t)scan * A.n_az * A.n_bins * A.stride;
  const long long r0 = (long long)row * A.n_bins;
  const unsigned rec = PACKED ? 16u : 4u * (unsigned)A.stride;          // bytes per point
  const char* rb = reinterpret_cast<const char*>(base + r0 * A.stride);  // uniform; lane offsets within a row fit 32 bits

  // the row's first point (a uniform address: one scalar load)
  const float x0 = reinterpret_cast<const float*>(rb)[0], y0 = reinterpret_cast<const float*>(rb)[1];
  RowWalk W(x0, y0);
  const bool near_cut = W.near_cut();
  // lane t holds bins t, t + 256, ...: FILT_UNROLL loads per lane and round, all issued before the first is looked at (rows
  // beyond 3072 bins take further rounds)
  for (int c0 = 0; c0 < A.n_bins; c0 += FILT_UNROLL * FILT_BLOCK) {
    float4 pt[FILT_UNROLL];
#pragma unroll
    for (int u = 0; u < FILT_UNROLL; ++u) {  // bins past the end of the row re-read its last bin and are skipped when visited
      const int b0 = c0 + u * FILT_BLOCK + tid;
      const unsigned off = (unsigned)(b0 < A.n_bins ? b0 : A.n_bins - 1) * rec;
      if (PACKED) {
        pt[u] = *reinterpret_cast<const float4*>(rb + off);
      } else {
        const float* p = reinterpret_cast<const float*>(rb + off);
        pt[u].x = p[0];
        pt[u].y = p[1];
        pt[u].w = p[A.ioff];
      }
    }
#pragma unroll
    for (int u = 0; u < FILT_UNROLL; ++u) {
      const int b = c0 + u * FILT_BLOCK + tid;
      if (PACKED) asm volatile("" ::"v"(pt[u].z));  // keeps the record ONE dwordx4 load (z is not needed here: the compiler would split it in two)
      if (b < A.n_bins) W.visit(A, b, pt[u].x, pt[u].y, (!PACKED || I3) ? pt[u].w : (A.ioff == 2 ? pt[u].z : (A.ioff == 1 ? pt[u].y : pt[u].x)));
    }
  }
  W.reduce_wave();
  float best_i = W.best_i;
  int best_idx = W.best_idx;
  const int flagged = __ballot(W.suspect) != 0ull ? 1 : 0;
  if (lane == 0) {
    s_best[wave] = best_i;
    s_idx[wave] = best_idx;
    s_flag[wave] = flagged;
  }
  __syncthreads();
  int any_flag = 0;
  best_i = s_best[0];
  best_idx = s_idx[0];
#pragma unroll
  for (int w = 0; w < FILT_WAVES; ++w) {
    any_flag |= s_flag[w];
    if (w > 0 && (s_best[w] > best_i || (s_best[w] == best_i && s_idx[w] < best_idx))) {
      best_i = s_best[w];
      best_idx = s_idx[w];
    }
  }
  int bad = 0;
  float a0 = 0.f;
  if (any_flag || near_cut) {  // uniform over the workgroup
    // the exact organisation test (rare: the row at the +-pi cut, and clouds that are not organised azimuth after azimuth):
    // the row once more, eight loads in flight per lane
    a0 = atan2f(y0, x0);
    const bool cut = !(fabsf(a0) < 3.14f);
    for (int c0 = 0; c0 < A.n_bins; c0 += 8 * FILT_BLOCK) {
      float qx[8], qy[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b0 = c0 + u * FILT_BLOCK + tid;
        const float* q = reinterpret_cast<const float*>(rb + (unsigned)(b0 < A.n_bins ? b0 : A.n_bins - 1) * rec);
        qx[u] = q[0];
        qy[u] = q[1];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c0 + u * FILT_BLOCK + tid < A.n_bins && W.exact_change(a0, cut, qx[u], qy[u])) bad = 1;
    }
    bad = __syncthreads_or(bad);
  }
  if (wave != 0) return;
  if (!(any_flag || near_cut)) a0 = atan2f(y0, x0);
  finish_row<PACKED ? SRC_PACKED : SRC_STRIDED>(A, scan_src<PACKED ? SRC_PACKED : SRC_STRIDED>(A, scan), g, row, best_i, best_idx, a0, bad, lane);
}

// The row kernel of a RASTER scan: ONE WAVEFRONT per azimuth row, 16 bytes of the raster per lane and load = 16 / 8 / 4 bins
// for u8 / u16 / f32 (ELEM: the RANDT_RASTER_* code).  A Navtech row (3768 u8 bins) is four loads of the wavefront and a whole
// scan 1.5 MB, so a launch is a chain of dependent rounds, not a stream: the raster loads of a round and the loads of the bins'
// ranges (a 15 KB table that every row shares, so it lives in the caches; independent of the raster values) are all issued
// before the first is looked at, the row's (cos, sin) is two scalars, and no barrier or LDS is needed -- the wavefront that found
// the arg-max expands the run itself.  The per-bin steps are k_filter_rows's, on x = ranges[b] * c, y = ranges[b] * s and
// I = (float)v * iscale: a lane meets its bins in increasing order (strict '>' keeps the first), lanes are combined towards the
// smaller index.  Bins past n_bins inside the last 16 bytes of a pitched row are loaded (the pitch is a multiple of 16, so the
// load stays inside the row) and never looked at.
// Measured against the cloud kernels on the expansion (400 x 3768 u8, profiles/r07_polar_raster_probe.json): 59.6 against 71.2 us
// per 16 scans, but 17.4 against 14.1 us for ONE scan per launch -- neither bytes nor the per-bin arithmetic bound it
// (profiles/experiments/r07_filter_raster_geometry.md: what was tried, and what is open).
#define FILT_RBLOCK 64
template <int ELEM>
__global__ __launch_bounds__(FILT_RBLOCK) void k_filter_raster_rows(FilterArgs A) {
  constexpr int ESZ = ELEM == RANDT_RASTER_U8 ? 1 : (ELEM == RANDT_RASTER_U16 ? 2 : 4);
  constexpr int EPL = 16 / ESZ;                            // bins per lane and load
  constexpr int RU = ELEM == RANDT_RASTER_U8 ? 4 : 8;      // loads per lane and round
  const int lane = threadIdx.x;
  const long long g = blockIdx.x;  // scan * n_az + row
  const int scan = (int)(g / A.n_az), row = (int)(g - (long long)scan * A.n_az);
  const ScanSrc S = scan_src<SRC_RASTER>(A, scan);
  const unsigned char* rb = S.ras + (size_t)row * A.row_pitch;  // uniform
  const float c = S.cs[2 * row], s = S.cs[2 * row + 1];
  const float* __restrict__ rng = A.ranges;
  const int nb = A.n_bins;

  // the row's first point, as the cloud path reads it from the expansion
  const float x0 = rng[0] * c, y0 = rng[0] * s;
  RowWalk W(x0, y0);
  for (int c0 = 0; c0 < nb; c0 += RU * FILT_RBLOCK * EPL) {
    uint4 q[RU];
    float rg[RU][EPL];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b0 = c0 + (u * FILT_RBLOCK + lane) * EPL;
      // a load that starts past the row re-reads the row's first 16 bytes and is skipped when visited
      q[u] = *reinterpret_cast<const uint4*>(rb + (b0 < nb ? (size_t)b0 * ESZ : (size_t)0));
#pragma unroll
      for (int k = 0; k < EPL; k += 4) {
        const int b = b0 + k;
        if (A.rng_vec && b + 3 < nb) {
          const float4 r4 = *reinterpret_cast<const float4*>(rng + b);
          rg[u][k] = r4.x, rg[u][k + 1] = r4.y, rg[u][k + 2] = r4.z, rg[u][k + 3] = r4.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) rg[u][k + e] = rng[b + e < nb ? b + e : nb - 1];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int b0 = c0 + (u * FILT_RBLOCK + lane) * EPL;
      const unsigned w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        float v;
        if (ELEM == RANDT_RASTER_U8) v = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        else if (ELEM == RANDT_RASTER_U16) v = (float)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
        else v = __uint_as_float(w[k]);
        if (b0 + k < nb) W.visit(A, b0 + k, rg[u][k] * c, rg[u][k] * s, v * A.iscale);
      }
    }
  }
  W.reduce_wave();
  int bad = 0;
  const float a0 = atan2f(y0, x0);
  if (__ballot(W.suspect) != 0ull || W.near_cut()) {  // uniform over the wavefront
    // the exact organisation test (the tables alone decide it: the raster is not read again)
    const bool cut = !(fabsf(a0) < 3.14f);
    for (int b = lane; b < nb; b += FILT_RBLOCK)
      if (W.exact_change(a0, cut, rng[b] * c, rng[b] * s)) bad = 1;
    bad = __ballot(bad != 0) != 0ull ? 1 : 0;
  }
  finish_row<SRC_RASTER>(A, S, g, row, W.best_i, W.best_idx, a0, bad, lane);
}

}  // namespace

namespace {
// host twin of hypot_f (glibc: correctly rounded double sqrt, one rounding to float)
inline float hypot_from_d2(double d2) { return (float)sqrt(d2); }
// smallest non-negative double d2 with pred(d2) true, for a predicate that is monotone (false ... true) in d2
template <typename Pred>
double first_true(Pred pred) {
  unsigned long long lo = 0, hi = 0x7ff0000000000000ull;  // bit patterns of +0 .. +inf are ordered like the values
  if (pred(0.0)) return 0.0;
  if (!pred(INFINITY)) return NAN;  // never true: every comparison with the threshold is false
  while (hi - lo > 1) {
    const unsigned long long mid = lo + (hi - lo) / 2;
    double v;
    memcpy(&v, &mid, 8);
    if (pred(v)) hi = mid; else lo = mid;
  }
  double v;
  memcpy(&v, &hi, 8);
  return v;
}
}  // namespace

namespace {
// everything of the kernels' arguments that does not depend on where the points come from
int filter_args(randt_ctx* ctx, FilterArgs& A, int n_scans, int n_az, int n_bins, const randt_filter_params* fp, float* d_out_pts, int pitch_out,
                int32_t* d_out_counts, float* d_polar, float* d_peaks, int32_t* d_peak_counts, int32_t* d_status, void* d_scratch) {
  memset(&A, 0, sizeof(A));
  A.n_scans = n_scans;
  A.n_az = n_az;
  A.n_bins = n_bins;
  A.min_d = fp->min_range;
  A.max_d = fp->max_range;
  A.min_i = fp->min_intensity;
  A.thr = fp->beam_distance_increment_threshold;
  {
    const float mn = A.min_d, mx = A.max_d;
    A.lo2 = first_true([mn](double d2) { return (double)hypot_from_d2(d2) > (double)mn; });
    // largest d2 still below max_d = predecessor of the first d2 that is not
    const double first_not_below = first_true([mx](double d2) { return !((double)hypot_from_d2(d2) < (double)mx); });
    A.hi2 = first_not_below > 0.0 ? nextafter(first_not_below, -1.0) : (first_not_below == 0.0 ? -1.0 : (double)INFINITY);
  }
  for (int i = 0; i < 12; ++i) A.T[i] = fp->sensor_to_base[i];
  A.out_pts = d_out_pts;
  A.out_polar = d_polar;
  A.peaks = d_peaks;
  A.out_counts = d_out_counts;
  A.peak_counts = d_peak_counts;
  A.status = d_status;
  A.pitch_out = pitch_out;
  A.out_vec = ((uintptr_t)d_out_pts & 15) == 0;
  A.rows = (RowRec*)d_scratch;  // [n_scans * n_az] records, then the stage (api.hip sizes the workspace: FILT_WS_PER_ROW)
  A.stage = (float4*)((char*)d_scratch + (((size_t)n_scans * n_az * sizeof(RowRec) + 255) & ~(size_t)255));
  if ((long long)n_scans * n_az > 0x7fffffffll) return randt_set_error(ctx, RANDT_ERR_UNSUPPORTED, "filter: more than 2^31 azimuth rows in one launch", hipSuccess);
  return RANDT_OK;
}
}  // namespace

int launch_filter_scan(randt_ctx* ctx, const float* d_raw, int n_scans, int n_az, int n_bins, int stride, int ioff,
                       const randt_filter_params* fp, float* d_out_pts, int pitch_out, int32_t* d_out_counts, float* d_polar,
                       float* d_peaks, int32_t* d_peak_counts, int32_t* d_status, void* d_scratch) {
  randt_note_enqueue(ctx);  // (RANDT_SOLVE_AUTO of the process's other contexts: this one has work in flight)
  FilterArgs A;
  const int rc = filter_args(ctx, A, n_scans, n_az, n_bins, fp, d_out_pts, pitch_out, d_out_counts, d_polar, d_peaks, d_peak_counts, d_status, d_scratch);
  if (rc) return rc;
  A.raw = d_raw;
  A.stride = stride;
  A.ioff = ioff;
  // one workgroup per azimuth row; the dispatcher back-fills the chip as workgroups retire
  const int row_wgs = n_scans * n_az;
  if (stride == 4 && ioff == 3) {
    hipLaunchKernelGGL((k_filter_rows<true, true>), dim3(row_wgs), dim3(FILT_BLOCK), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_filter_emit<SRC_PACKED>, dim3(n_scans), dim3(FILT_EBLOCK), 0, ctx->stream, A);
  } else if (stride == 4) {
    hipLaunchKernelGGL((k_filter_rows<true, false>), dim3(row_wgs), dim3(FILT_BLOCK), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_filter_emit<SRC_PACKED>, dim3(n_scans), dim3(FILT_EBLOCK), 0, ctx->stream, A);
  } else {
    hipLaunchKernelGGL((k_filter_rows<false, false>), dim3(row_wgs), dim3(FILT_BLOCK), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_filter_emit<SRC_STRIDED>, dim3(n_scans), dim3(FILT_EBLOCK), 0, ctx->stream, A);
  }
  RANDT_HIP_CHECK(ctx, hipGetLastError());
  return RANDT_OK;
}

// The same two steps for raster scans (randt_filter_raster_batch_dev, which has validated descriptor and alignment): one
// wavefront per azimuth row, then the emission over the same row records.
int launch_filter_raster(randt_ctx* ctx, const void* d_raster, const randt_polar_raster* desc, const float* d_cossin, const float* d_ranges,
                         int n_scans, const randt_filter_params* fp, float* d_out_pts, int pitch_out, int32_t* d_out_counts, float* d_polar,
                         float* d_peaks, int32_t* d_peak_counts, int32_t* d_status, void* d_scratch) {
  randt_note_enqueue(ctx);
  FilterArgs A;
  const int rc = filter_args(ctx, A, n_scans, desc->n_azimuths, desc->n_bins, fp, d_out_pts, pitch_out, d_out_counts, d_polar, d_peaks, d_peak_counts,
                             d_status, d_scratch);
  if (rc) return rc;
  A.stride = 4;  // (the expansion's; no kernel of this path reads them)
  A.ioff = 3;
  A.raster = static_cast<const unsigned char*>(d_raster);
  A.cossin = d_cossin;
  A.ranges = d_ranges;
  A.row_pitch = desc->row_pitch_bytes;
  A.scan_pitch = desc->scan_pitch_bytes;
  A.iscale = desc->intensity_scale;
  A.elem = desc->elem_type;
  A.rng_vec = ((uintptr_t)d_ranges & 15) == 0;
  const dim3 grid(n_scans * desc->n_azimuths), block(FILT_RBLOCK);
  if (A.elem == RANDT_RASTER_U8) hipLaunchKernelGGL(k_filter_raster_rows<RANDT_RASTER_U8>, grid, block, 0, ctx->stream, A);
  else if (A.elem == RANDT_RASTER_U16) hipLaunchKernelGGL(k_filter_raster_rows<RANDT_RASTER_U16>, grid, block, 0, ctx->stream, A);
  else hipLaunchKernelGGL(k_filter_raster_rows<RANDT_RASTER_F32>, grid, block, 0, ctx->stream, A);
  hipLaunchKernelGGL(k_filter_emit<SRC_RASTER>, dim3(n_scans), dim3(FILT_EBLOCK), 0, ctx->stream, A);
  RANDT_HIP_CHECK(ctx, hipGetLastError());
  return RANDT_OK;
}
