// f-3 for many pairs at once: Matcher::estimateTransformGlobalBNB (ndt_matcher.cpp:495-608) with the level loop on the device.
// randt_search_global (api.hip) replays the reference's FIFO on the host, one synchronisation per level; here the host
// enqueues, blindly, per level one evaluation launch over every (pair, node) and one expansion launch with a workgroup per
// pair, and reads nothing back.  The answers are the single call's bit for bit:
//   - everything libm touches (cos / sin of the grid angles, acos, pow, the running sums of the grid loops) is computed by
//     the host and arrives as tables of delta poses; the device forms node = parent x delta with se2_mul_host below, the
//     operation-for-operation copy of h_se2_mul / h_so2_normalize (under `fp contract(off)`: the host object has no fused
//     operations);
//   - a pose's cost comes from k_eval_cost_pairs below: k_eval_cost (solve.hip) statement for statement, on the inlined
//     functions of solve_math.h, compiled with the flags of solve.hip (the Makefile gives this file no -ffp-contract=off; the
//     exact parts carry their own pragma), with the pair / node indirection in front.  The compiler's choice of fused
//     operations is part of the result: tests/test_gpu_search_batch.py holds batch and single call to the same bits;
//   - the reference drops a child whose nine-float key was generated before.  Of the nine only (float)c, (float)s, (float)tx,
//     (float)ty vary, and float == is transitive apart from NaN (which equals nothing on either path), so "found among the
//     keys inserted so far" is "equals no earlier inserted key": the key table holds the inserted nodes in FIFO order, a
//     level is a contiguous range of it, and children are checked and appended in FIFO order, a block at a time.
#include "randt_internal.h"
#include "solve_math.h"

using namespace randt_solve;

namespace {

constexpr int BLOCK = 1024;
constexpr int WAVES = BLOCK / RANDT_WAVE;

// h_se2_mul (api.hip) = Sophus SO2 product with its renormalisation, then the translation
__device__ __forceinline__ void se2_mul_host(const double* a, const double* b, double* out) {
#pragma clang fp contract(off)
  double re = a[0] * b[0] - a[1] * b[1];
  double im = a[0] * b[1] + a[1] * b[0];
  const double sq = re * re + im * im;
  if (sq != 1.0) {
    const double scale = 2.0 / (1.0 + sq);
    re *= scale;
    im *= scale;
  }
  const double len = sqrt(re * re + im * im);
  re = re / len;
  im = im / len;
  out[0] = re;
  out[1] = im;
  out[2] = a[2] + (a[0] * b[2] - a[1] * b[3]);
  out[3] = a[3] + (a[1] * b[2] + a[0] * b[3]);
}

__device__ __forceinline__ float4 key_of(const double* p) { return make_float4((float)p[0], (float)p[1], (float)p[2], (float)p[3]); }
__device__ __forceinline__ bool same_key(const float4& a, const float4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// level 1: node i of a pair = guess x delta i of the pair's grid; every one is inserted (the reference does not look them up)
__global__ __launch_bounds__(256) void k_bnb_seed(const double* __restrict__ guess4, const int2* __restrict__ pair_table,
                                                  const double* __restrict__ level1, int max_nodes, double* __restrict__ poses,
                                                  float4* __restrict__ keys, int2* __restrict__ level, BnbState* __restrict__ state) {
  const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int2 tab = pair_table[pair];
  const bool overflow = tab.y > max_nodes;
  if (i == 0) {
    level[pair] = make_int2(0, overflow ? 0 : tab.y);
    BnbState st;
    st.min_cost = 100000.0;
    st.best[0] = 1.0; st.best[1] = 0.0; st.best[2] = 0.0; st.best[3] = 0.0;
    st.n_evals = 0;
    st.status = overflow ? 1 : 0;
    state[pair] = st;
  }
  if (overflow || i >= tab.y) return;
  double g[4], d[4], x[4];
  for (int c = 0; c < 4; ++c) {
    g[c] = guess4[4 * (size_t)pair + c];
    d[c] = level1[4 * ((size_t)tab.x + i) + c];
  }
  se2_mul_host(g, d, x);
  const size_t node = (size_t)pair * max_nodes + i;
  for (int c = 0; c < 4; ++c) poses[4 * node + c] = x[c];
  keys[node] = key_of(x);
}

// k_eval_cost of solve.hip for many pairs: blockIdx.y is the pair -- fixed map fixed_idx[pair], moving map moving_first + pair,
// its own correspondence table, and of its node_stride rows of poses4 / cost the nodes [level.x, level.x + level.y), read on
// the device; a wavefront beyond the pair's live count leaves before it touches the maps.  From `const Loss L` on this IS
// k_eval_cost: keep the two identical.
template <int D>
__global__ __launch_bounds__(64) void k_eval_cost_pairs(MapView fixed, const int32_t* __restrict__ fixed_idx, MapView moving, int moving_first,
                                                        const int32_t* __restrict__ corr_all, int k, double scale, double alpha,
                                                        const double* __restrict__ poses_all, double* __restrict__ cost_all,
                                                        int32_t* __restrict__ n_res_out, const int2* __restrict__ level, int node_stride) {
  const int pair = blockIdx.y, lane = threadIdx.x;
  const int2 lv = level[pair];
  if ((int)blockIdx.x >= lv.y) return;
  const int p = lv.x + blockIdx.x;
  const int fmap = fixed_idx[pair], mmap = moving_first + pair;
  const int32_t* corr = corr_all + (size_t)pair * moving.cap * k;
  const double* poses4 = poses_all + 4 * (size_t)pair * node_stride;
  double* cost = cost_all + (size_t)pair * node_stride;
  int M = moving.counts[mmap];
  M = M > moving.cap ? moving.cap : M;
  const float4* mov = reinterpret_cast<const float4*>(moving.cells + (size_t)mmap * moving.cap);
  const float4* fix = reinterpret_cast<const float4*>(fixed.cells + (size_t)fmap * fixed.cap);
  const Loss L = make_loss(scale, alpha, 1.0, 1.0);  // BarronLoss(scale, alpha): b = a^2, no ScaledLoss (:517)
  const double* x = poses4 + 4 * (size_t)p;
  const double inv = rsqrt(x[0] * x[0] + x[1] * x[1]);
  const double c = x[0] * inv, s = x[1] * inv, tx = x[2], ty = x[3];
  const Rot rot = make_rot(c, s);
  double acc = 0.0;
  int n = 0;
  for (int slot = lane; slot < M * k; slot += 64) {
    const int ci = corr[slot];
    if (ci < 0 || ci >= fixed.cap) continue;
    double jb[3];
    const double sq = residual_sq<D, false>(mov + (size_t)(slot / k) * 3, fix + (size_t)ci * 3, rot, tx, ty, jb);
    ++n;
    if (L.mode == 2) {
      const double iu = 1.0 / (sq * L.ts + 1.0);
      acc += L.half_w_pre * (iu - 1.);
    } else {
      double r0, r1, r2;
      loss_eval(L, sq, r0, r1, r2);
      acc += 0.5 * r0;
    }
  }
  acc = wave_sum(acc);
  const double nn = wave_sum((double)n);
  if (lane == 0) {
    cost[p] = acc;
    if (blockIdx.x == 0) n_res_out[pair] = (int)nn;
  }
}

// exclusive rank of `flag` among the workgroup's threads, and the total; s_w: WAVES + 1 words
__device__ __forceinline__ int block_rank(bool flag, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  __syncthreads();  // the previous use of s_w is over
  if (lane == 0) s_w[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < WAVES; ++w) {
    const int n = s_w[w];
    before += w < wave ? n : 0;
    all += n;
  }
  *total = all;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

// One level of one pair: threshold, minimum, children, dedupe, the next level's range.  `last`: the call's final launch, which
// writes the answers.  A pair that has run out of nodes only passes through.
__global__ __launch_bounds__(BLOCK) void k_bnb_expand(int level_no, int n_iter, double threshold, const double* __restrict__ children,
                                                      int max_nodes, double* poses_all, float4* keys_all, const double* __restrict__ cost_all,
                                                      int32_t* admitted_all, const int32_t* __restrict__ n_res, int2* level, BnbState* state,
                                                      int last, double* trans4, randt_bnb_result* results) {
#pragma clang fp contract(off)
  __shared__ float4 s_keys[BLOCK];
  __shared__ int s_w[WAVES + 1];
  __shared__ double s_cost[WAVES];
  __shared__ int s_idx[WAVES];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int2 lv = level[pair];
  const int begin = lv.x, count = lv.y;
  double* poses = poses_all + 4 * (size_t)pair * max_nodes;
  float4* keys = keys_all + (size_t)pair * max_nodes;
  const double* cost = cost_all + (size_t)pair * max_nodes;
  int32_t* admitted = admitted_all + (size_t)pair * max_nodes;
  if (count > 0) {
    const bool descend = level_no < n_iter;
    const double nres = (double)n_res[pair];
    // the FIFO's `current_cost < threshold`, `current_cost < min_cost`: the first node of the smallest admitted cost
    double my_cost = 0.0;
    int my_idx = -1, n_adm = 0;
    for (int base = 0; base < count; base += BLOCK) {
      const int i = base + tid;
      bool adm = false;
      if (i < count) {
        const double cc = cost[begin + i] / nres;
        adm = cc < threshold;
        if (adm && (my_idx < 0 || cc < my_cost)) {
          my_cost = cc;
          my_idx = i;
        }
      }
      if (descend) {
        int total;
        const int r = block_rank(adm, s_w, &total);
        if (adm) admitted[n_adm + r] = i;
        n_adm += total;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double oc = __shfl_xor(my_cost, off);
      const int oi = __shfl_xor(my_idx, off);
      if (oi >= 0 && (my_idx < 0 || oc < my_cost || (oc == my_cost && oi < my_idx))) {
        my_cost = oc;
        my_idx = oi;
      }
    }
    if ((tid & 63) == 0) {
      s_cost[tid >> 6] = my_cost;
      s_idx[tid >> 6] = my_idx;
    }
    __syncthreads();  // also: admitted[] is written
    if (tid == 0) {
      for (int w = 1; w < WAVES; ++w)
        if (s_idx[w] >= 0 && (my_idx < 0 || s_cost[w] < my_cost || (s_cost[w] == my_cost && s_idx[w] < my_idx))) {
          my_cost = s_cost[w];
          my_idx = s_idx[w];
        }
      BnbState& st = state[pair];
      st.n_evals += count;
      if (my_idx >= 0 && my_cost < st.min_cost) {
        st.min_cost = my_cost;
        for (int c = 0; c < 4; ++c) st.best[c] = poses[4 * (size_t)(begin + my_idx) + c];
      }
    }
    // 27 children per admitted node, in FIFO order, a block at a time against the table so far and the block's earlier ones
    int table = begin + count;
    bool overflow = false;
    const long long n_children = 27ll * n_adm;
    const double* delta = children + 4 * 27 * (size_t)(level_no - 1);
    for (long long base = 0; base < n_children; base += BLOCK) {
      const long long c = base + tid;
      const bool valid = c < n_children;
      double x[4] = {0.0, 0.0, 0.0, 0.0};
      float4 key = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) {
        const int parent = admitted[c / 27], j = (int)(c % 27);
        double a[4], d[4];
        for (int q = 0; q < 4; ++q) {
          a[q] = poses[4 * (size_t)(begin + parent) + q];
          d[q] = delta[4 * j + q];
        }
        se2_mul_host(a, d, x);
        key = key_of(x);
      }
      s_keys[tid] = key;
      __syncthreads();
      bool found = false;
      if (valid) {
        for (int t = 0; t < table; ++t) found |= same_key(keys[t], key);
        for (int t = 0; t < tid; ++t) found |= same_key(s_keys[t], key);
      }
      const bool survive = valid && !found;
      int total;
      const int r = block_rank(survive, s_w, &total);
      if (table + total > max_nodes) {  // uniform
        overflow = true;
        break;
      }
      if (survive) {
        keys[table + r] = key;
        for (int q = 0; q < 4; ++q) poses[4 * (size_t)(table + r) + q] = x[q];
      }
      table += total;
      __syncthreads();  // the appended keys are the next block's table; s_keys is free
    }
    if (tid == 0) {
      level[pair] = overflow ? make_int2(0, 0) : make_int2(begin + count, table - (begin + count));
      if (overflow) state[pair].status = 1;
    }
  }
  if (last && tid == 0) {
    const BnbState st = state[pair];  // this thread wrote it
    randt_bnb_result r;
    r.min_cost = st.min_cost;
    r.n_evals = st.n_evals;
    r.status = st.status;
    results[pair] = r;
    if (st.status == 0)
      for (int c = 0; c < 4; ++c) trans4[4 * (size_t)pair + c] = st.best[c];
  }
}

}  // namespace

int launch_search_global_batch(randt_ctx* ctx, const MapView& fixed, const MapView& moving, const BnbBatch& b) {
  // at least one block per pair: thread 0 of block 0 sets the pair's state and level, whatever its grid (empty, or over max_nodes)
  const int seed_blocks = b.level1_bound > 0 ? (b.level1_bound + 255) / 256 : 1;
  hipLaunchKernelGGL(k_bnb_seed, dim3(seed_blocks, b.n_pairs), dim3(256), 0, ctx->stream, b.trans4, b.pair_table, b.level1, b.max_nodes,
                     b.poses, reinterpret_cast<float4*>(b.keys), b.level, b.state);
  RANDT_HIP_CHECK(ctx, hipGetLastError());
  // association once at the guess, frozen for the search (quirk A.7-8); the guesses are still in trans4
  int rc = launch_associate(ctx, fixed, b.fixed_idx, moving, b.moving_first, b.n_pairs, b.trans4, b.k, b.lookup_mahalanobis,
                            b.use_intensity, b.corr);
  if (rc) return rc;
  long long bound = b.level1_bound;  // nodes a pair can have at this level: level 1 is exact
  for (int level_no = 1; level_no <= b.n_iter; ++level_no) {
    if (bound > b.max_nodes) bound = b.max_nodes;
    if (bound > 0) {
      const dim3 grid((unsigned)bound, b.n_pairs);
      if (b.use_intensity)
        hipLaunchKernelGGL(k_eval_cost_pairs<3>, grid, dim3(64), 0, ctx->stream, fixed, b.fixed_idx, moving, b.moving_first, b.corr, b.k, b.scale,
                           b.alpha, b.poses, b.cost, b.n_res, b.level, b.max_nodes);
      else
        hipLaunchKernelGGL(k_eval_cost_pairs<2>, grid, dim3(64), 0, ctx->stream, fixed, b.fixed_idx, moving, b.moving_first, b.corr, b.k, b.scale,
                           b.alpha, b.poses, b.cost, b.n_res, b.level, b.max_nodes);
      RANDT_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_bnb_expand, dim3(b.n_pairs), dim3(BLOCK), 0, ctx->stream, level_no, b.n_iter, b.threshold, b.children, b.max_nodes,
                       b.poses, reinterpret_cast<float4*>(b.keys), b.cost, b.admitted, b.n_res, b.level, b.state,
                       level_no == b.n_iter ? 1 : 0, b.trans4, b.results);
    RANDT_HIP_CHECK(ctx, hipGetLastError());
    bound *= 27;
  }
  return RANDT_OK;
}
