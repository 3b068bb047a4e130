// What the Scan Context translation units share: scancontext.hip (loop closure inside one database) and
// scancontext_query.hip (a query from outside the database).  Device code only; both files are compiled with
// -ffp-contract=off, and every sum below is one thread's left-to-right loop in the reference's order, so a (query, candidate)
// pair gets the same bits from either file.
#pragma once
#include "randt_internal.h"

#include <math.h>

#pragma clang fp contract(off)

// The limits live in scancontext.hip (the tests parse them out of that file); a unit that does not state them gets them here,
// and a restatement that disagrees does not compile.
#ifndef SC_BLOCK
#define SC_BLOCK 256
#define SC_MAX_SECTOR 128
#define SC_MAX_RING 64
#define SC_MAX_CAND 32
#define SC_TERM_CAP 4096
#endif
static_assert(SC_BLOCK == 256 && SC_MAX_SECTOR == 128 && SC_MAX_RING == 64 && SC_MAX_CAND == 32 && SC_TERM_CAP == 4096,
              "the Scan Context limits are stated twice (scancontext.hip, scancontext_shared.h): keep them equal");

namespace {

struct ScParams {
  int R, S, exclude_recent, n_cand, radius;
  double max_radius, dist_thresh, assumed_drift, odom_eps, odom_weight, intensity_factor;
};

// what a (query, candidate) workgroup leaves for the pick kernel
struct ScCandidate {
  double cd;           // distanceBtnScanContext + the odometry term
  int32_t shift, idx;  // argmin shift, database index (-1: this query has fewer candidates)
};

inline ScParams to_dev(const randt_sc_params* p) {
  ScParams P;
  P.R = p->num_ring;
  P.S = p->num_sector;
  P.exclude_recent = p->num_exclude_recent;
  P.n_cand = p->num_candidates;
  P.radius = (int)round(0.5 * p->search_ratio * p->num_sector);
  P.max_radius = p->max_radius;
  P.dist_thresh = p->dist_thresh;
  P.assumed_drift = p->assumed_drift;
  P.odom_eps = p->odom_eps;
  P.odom_weight = p->odom_weight;
  P.intensity_factor = p->intensity_factor;
  return P;
}

// lexicographic (value, index) block arg-min over 256 threads; result broadcast.  scratch: 2 x 4 words.
__device__ __forceinline__ void block_argmin(double& v, int& idx, double* sv, int* si) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    if (ov < v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
  __syncthreads();
  if (lane == 0) {
    sv[wave] = v;
    si[wave] = idx;
  }
  __syncthreads();
  v = sv[0];
  idx = si[0];
#pragma unroll
  for (int w = 1; w < SC_BLOCK / 64; ++w)
    if (sv[w] < v || (sv[w] == v && si[w] < idx)) {
      v = sv[w];
      idx = si[w];
    }
}

// the reference's return value for an argmin shift (Scancontext.cpp:336): deg2rad of a float angle, in double
__device__ __forceinline__ float sc_shift_yaw(int shift, int S) { return (float)((float)(shift * (360.0 / (double)S)) * M_PI / 180.0); }

// the odometry term of distanceBtnScanContext (:140-152) between a query (pos1, dist1) and a candidate (pos2, dist2)
__device__ __forceinline__ double sc_odom_term(const ScParams& P, double x1, double y1, double d1, double x2, double y2, double d2) {
  const double dx = x2 - x1, dy = y2 - y1;
  double t_err = sqrt(dx * dx + dy * dy) - P.odom_eps;
  t_err = (t_err > 0.0 ? t_err : 0.0) / (d2 - d1);
  return 1 - exp(-(t_err * t_err) / (2 * P.assumed_drift * P.assumed_drift));
}

// distanceBtnScanContext without the odometry term (:115-139) for one (query, candidate) pair, by a whole workgroup of
// SC_BLOCK threads: sector-key alignment, then the column-shift search of the cosine distance.  Every thread returns with the
// argmin shift and the minimal distance.
//   staged          the two descriptors (S x R doubles each) are copied into the dynamic LDS with coalesced loads; every dot
//                   product below then reads LDS instead of walking two global columns element by element (a candidate cost
//                   12 us of L2 round trips that way).  Descriptors too large for it stay in global memory;
//   spread_shifts   the (shift, column) cosine terms fit `term`: all threads form them, see below.
__device__ __forceinline__ void sc_descriptor_distance(const ScParams& P, const double* sc1, const double* sc2, int staged, bool spread_shifts,
                                                       int& argmin_shift, double& min_sc) {
  extern __shared__ __attribute__((aligned(16))) char sc_dyn[];
  __shared__ double k1[SC_MAX_SECTOR], k2[SC_MAX_SECTOR];
  __shared__ double n1[SC_MAX_SECTOR], n2[SC_MAX_SECTOR];  // column norms of the query / the candidate (shift-independent)
  __shared__ double term[SC_TERM_CAP];
  __shared__ double sv[4];
  __shared__ int si[4];
  const int tid = threadIdx.x;
  const int R = P.R, S = P.S;
  // ---- pairwise distances (distanceBtnScanContext) in candidate order
  double* s1 = reinterpret_cast<double*>(sc_dyn);
  double* s2 = s1 + (size_t)R * S;
  if (staged) {
    for (int i = tid; i < R * S; i += SC_BLOCK) s1[i] = sc1[i];
    __syncthreads();
    sc1 = s1;
  }
  // The column-shift search evaluates, per shift, sum over the columns of dot / (|a| |b|): the norms do not depend on the shift
  // and the (shift, column) dot products not on each other, so they are formed once / by all 256 threads; only each shift's sum
  // over the columns stays one thread's left-to-right loop (the reference's order) -- same numbers, ~30x less serial work.
  const int n_shift = 2 * P.radius + 1;
  if (tid < S) {
    double a = 0, na = 0;
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
      const double v = sc1[(size_t)tid * R + r];
      a += v;
      na += v * v;
    }
    k1[tid] = a / R;
    n1[tid] = sqrt(na);
  }
  __syncthreads();
  if (staged) {
    for (int i = tid; i < R * S; i += SC_BLOCK) s2[i] = sc2[i];
    __syncthreads();
    sc2 = s2;
  }
  if (tid < S) {
    double b = 0, nb = 0;
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
      const double v = sc2[(size_t)tid * R + r];
      b += v;
      nb += v * v;
    }
    k2[tid] = b / R;
    n2[tid] = sqrt(nb);
  }
  __syncthreads();
  // fastAlignUsingVkey: thread = shift, first minimal shift wins
  double nv = 1e300;
  int ns = 0x7fffffff;
  if (tid < S) {
    double nn = 0;
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
      int j = s - tid;
      j = j < 0 ? j + S : j;
      const double d = k1[s] - k2[j];
      nn += d * d;
    }
    nv = sqrt(nn);
    ns = tid;
    if (!(nv < 10000000)) {  // "cur_diff_norm < min" never true: shift 0 stays
      nv = 1e300;
      ns = 0x7fffffff;
    }
  }
  block_argmin(nv, ns, sv, si);
  const int argmin_vkey = ns == 0x7fffffff ? 0 : ns;
  // column-shift search: the 2 radius + 1 shifts around it, ascending shift value = thread order
  double dv = 1e300;
  int ds = 0x7fffffff;
  if (spread_shifts) {
    // every (shift slot, column) term by all threads; slot i holds shift argmin - radius + i (mod S)
    for (int p = tid; p < n_shift * S; p += SC_BLOCK) {
      const int slot = p / S, col = p - slot * S;
      int sh = argmin_vkey - P.radius + slot;
      sh = sh < 0 ? sh + S : (sh >= S ? sh - S : sh);
      int j = col - sh;
      j = j < 0 ? j + S : j;
      const double* a = sc1 + (size_t)col * R;
      const double* b = sc2 + (size_t)j * R;
      double dot = 0;
#pragma unroll 4
      for (int r = 0; r < R; ++r) dot += a[r] * b[r];
      const double na = n1[col], nb2 = n2[j];
      term[p] = (na == 0 || nb2 == 0) ? 1e300 : dot / (na * nb2);  // 1e300: the column is skipped
    }
    __syncthreads();
    if (tid < S) {
      int delta = tid - argmin_vkey;
      delta = delta < 0 ? delta + S : delta;
      const bool in = delta <= P.radius || S - delta <= P.radius;
      if (in) {
        const int slot = delta <= P.radius ? P.radius + delta : P.radius - (S - delta);
        int n_eff = 0;
        double sum = 0;
#pragma unroll 4
        for (int col = 0; col < S; ++col) {
          const double t = term[slot * S + col];
          if (t == 1e300) continue;
          sum = sum + t;
          n_eff = n_eff + 1;
        }
        const double d = 1.0 - sum / n_eff;
        if (d < 10000000) {  // NaN (no effective column) never wins, like "cur < min"
          dv = d;
          ds = tid;
        }
      }
    }
  } else if (tid < S) {
    // is shift `tid` in the search space {argmin + ii mod S, |ii| <= radius}?
    int delta = tid - argmin_vkey;
    delta = delta < 0 ? delta + S : delta;
    const bool in = delta <= P.radius || S - delta <= P.radius;
    if (in) {
      int n_eff = 0;
      double sum = 0;
      for (int col = 0; col < S; ++col) {
        int j = col - tid;
        j = j < 0 ? j + S : j;
        const double* a = sc1 + (size_t)col * R;
        const double* b = sc2 + (size_t)j * R;
        double na = 0, nb2 = 0, dot = 0;
        for (int r = 0; r < R; ++r) {
          na += a[r] * a[r];
          nb2 += b[r] * b[r];
          dot += a[r] * b[r];
        }
        na = sqrt(na);
        nb2 = sqrt(nb2);
        if (na == 0 || nb2 == 0) continue;
        sum = sum + dot / (na * nb2);
        n_eff = n_eff + 1;
      }
      const double d = 1.0 - sum / n_eff;
      if (d < 10000000) {  // NaN (no effective column) never wins, like "cur < min"
        dv = d;
        ds = tid;
      }
    }
  }
  block_argmin(dv, ds, sv, si);
  argmin_shift = ds == 0x7fffffff ? 0 : ds;
  min_sc = ds == 0x7fffffff ? 10000000 : dv;
}

}  // namespace
