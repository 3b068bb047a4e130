// Scan Context place recognition for a scan that is NOT a node of the database (compiled with -ffp-contract=off):
// relocalisation after a restart or a tracking loss, localisation in an earlier session's map.  detectLoopClosureID
// (Scancontext.cpp:261-341) with the query's descriptor, ring key and (optionally) odometry taken from arrays of their own,
// over ALL n_db nodes, and every candidate's record kept.
//
// The shape is the opposite of loop closure's (scancontext.hip: one query per keyframe, one workgroup per query): 1 .. 16
// queries against the largest database the process holds.  So the candidate search is spread over the chip:
//   k_scq_chunk   grid (query, chunk): the float ring-key distances of SCQ_CHUNK database entries (the numbers of k_sc_knn:
//                 nanoflann L2 on the float keys, accumulated ring by ring in float) from keys staged in LDS, then every entry's RANK inside
//                 its chunk by counting the entries that precede it in (distance, index) order -- no sequential arg-min
//                 rounds; the entries of rank < num_candidates go to their slot of the chunk's partial list;
//   k_scq_merge   grid (query): num_candidates (distance, index) arg-min rounds over the n_chunks x num_candidates partial
//                 entries.  A distance depends on its database entry alone and (distance, index) is a total order on the valid
//                 entries, so the k smallest of the chunks' k smallest ARE the k smallest of the database, ties included;
//   k_scq_detect  grid (query, rank): sc_descriptor_distance (scancontext_shared.h), k_sc_detect's arithmetic;
//   k_scq_pick    first smallest distance, and the per-candidate outputs.
// NaN rule (decision 13): an entry whose key distance is not >= 0 is never a candidate; +inf ranks last.
#include "scancontext_shared.h"

#define SCQ_CHUNK 512  // database entries per workgroup of the candidate search: see DESIGN, Scan Context, "query from outside"

namespace {

__global__ __launch_bounds__(SC_BLOCK) void k_scq_chunk(ScParams P, const double* __restrict__ ring_keys, int n_db,
                                                        const double* __restrict__ q_ring_keys, float* __restrict__ part_d,
                                                        int32_t* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) float keyf[];  // [SCQ_CHUNK][R | 1] the chunk's ring keys, rounded to float
  __shared__ float qk[SC_MAX_RING];
  __shared__ __attribute__((aligned(16))) float d2[SCQ_CHUNK];
  __shared__ int n_valid;
  const int q = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  const int R = P.R, k = P.n_cand;
  const int i0 = chunk * SCQ_CHUNK;
  const int len = n_db - i0 < SCQ_CHUNK ? n_db - i0 : SCQ_CHUNK;  // (>= 1: the grid has ceil(n_db / SCQ_CHUNK) chunks)
  if (tid < R) qk[tid] = (float)q_ring_keys[(size_t)q * R + tid];
  if (tid == 0) n_valid = 0;
  // The chunk's keys are one contiguous run of len x R doubles: read it with coalesced loads (independent of each other, so they
  // overlap) and keep the keys as floats in LDS, entry e at e * stride, stride odd so that the 64 lanes of a wavefront -- one
  // entry each -- hit 64 banks.  (A thread walking its own 8 R-byte row from global memory waited for every ring: 32 us a chunk.)
  const int stride = R | 1;
  {
    const double* __restrict__ run = ring_keys + (size_t)i0 * R;
    const int total = len * R;
#pragma unroll 8
    for (int t = tid; t < total; t += SC_BLOCK) {
      const int e = t / R;
      keyf[e * stride + (t - e * R)] = (float)run[t];
    }
  }
  __syncthreads();
  for (int j = tid; j < len; j += SC_BLOCK) {
    const float* key = keyf + j * stride;
    float acc = 0.0f;
    for (int r = 0; r < R; ++r) {
      const float a = qk[r], b = key[r];
      const float d = a - b;
      acc += d * d;
    }
    d2[j] = acc;
  }
  for (int j = len + tid; j < ((len + 3) & ~3); j += SC_BLOCK) d2[j] = NAN;  // the ranking reads whole float4s: the pad counts for nothing
  __syncthreads();
  float* pd = part_d + ((size_t)q * gridDim.y + chunk) * k;
  int32_t* pi = part_i + ((size_t)q * gridDim.y + chunk) * k;
  // rank of entry j = the entries that precede it in (distance, index) order.  A wavefront holds 64 consecutive entries, so for
  // all its lanes alike an entry in front of that block precedes on "<=" and one behind it on "<": one compare per pair,
  // wave-uniform loops; only the block's own 64 entries need the index test.  (NaN compares false: never counted, and the pad too.)
  int mine = 0;
  const float4* d4 = reinterpret_cast<const float4*>(d2);
  const int len4 = (len + 3) & ~3;
  for (int j0 = tid & ~63; j0 < len; j0 += SC_BLOCK) {
    const int j = j0 + (tid & 63);
    const float v = j < len ? d2[j] : NAN;
    const int j1 = j0 + 64 < len4 ? j0 + 64 : len4;
    int rank = 0;
#pragma unroll 4
    for (int m = 0; m < j0; m += 4) {  // (every lane reads the same words: LDS broadcasts, four entries per read)
      const float4 w = d4[m >> 2];
      rank += (w.x <= v ? 1 : 0) + (w.y <= v ? 1 : 0) + (w.z <= v ? 1 : 0) + (w.w <= v ? 1 : 0);
    }
    for (int m = j0; m < j1; m += 4) {
      const float4 w = d4[m >> 2];
      rank += (w.x < v || (w.x == v && m < j)) ? 1 : 0;
      rank += (w.y < v || (w.y == v && m + 1 < j)) ? 1 : 0;
      rank += (w.z < v || (w.z == v && m + 2 < j)) ? 1 : 0;
      rank += (w.w < v || (w.w == v && m + 3 < j)) ? 1 : 0;
    }
#pragma unroll 4
    for (int m = j1; m < len; m += 4) {
      const float4 w = d4[m >> 2];
      rank += (w.x < v ? 1 : 0) + (w.y < v ? 1 : 0) + (w.z < v ? 1 : 0) + (w.w < v ? 1 : 0);
    }
    if (!(v >= 0.0f)) continue;  // NaN (or beyond the chunk): never a candidate
    if (rank < k) {
      pd[rank] = v;
      pi[rank] = i0 + j;
    }
    ++mine;
  }
  if (mine) atomicAdd(&n_valid, mine);
  __syncthreads();
  // the slots no valid entry took (a distinct (distance, index) per entry: the ranks 0 .. n_valid - 1 are each taken once)
  if (tid < k && tid >= n_valid) {
    pd[tid] = -1.0f;
    pi[tid] = -1;
  }
}

__global__ __launch_bounds__(SC_BLOCK) void k_scq_merge(ScParams P, int n_part, float* __restrict__ part_d, const int32_t* __restrict__ part_i,
                                                        int32_t* __restrict__ cand_out) {
  __shared__ double sv[4];
  __shared__ int si[4];
  const int q = blockIdx.x, tid = threadIdx.x;
  float* pd = part_d + (size_t)q * n_part;
  const int32_t* pi = part_i + (size_t)q * n_part;
  int32_t* cand = cand_out + (size_t)q * P.n_cand;
  // A thread owns the slots tid, tid + SC_BLOCK, ...: nobody else reads or retires them, so its best entry stays its best until
  // it wins a round, and only the winner walks its slots again -- a round costs the others one block arg-min, no memory.
  double my_v = INFINITY;  // (a +inf distance IS >= 0 and is taken, lowest index first, by the == clause)
  int my_i = 0x7fffffff, my_slot = -1;
  bool rescan = true;
  for (int c = 0; c < P.n_cand; ++c) {
    if (rescan) {
      my_v = INFINITY;
      my_i = 0x7fffffff;
      my_slot = -1;
      for (int s = tid; s < n_part; s += SC_BLOCK) {
        const float v = pd[s];
        const int i = pi[s];
        if (v >= 0.0f && ((double)v < my_v || ((double)v == my_v && i < my_i))) {  // (an absent or retired slot holds -1)
          my_v = (double)v;
          my_i = i;
          my_slot = s;
        }
      }
    }
    double bv = my_v;
    int bi = my_i;
    block_argmin(bv, bi, sv, si);
    if (bi == 0x7fffffff) {  // uniform: nothing is left, this rank and every later one are absent
      if (tid == 0)
        for (int c2 = c; c2 < P.n_cand; ++c2) cand[c2] = -1;
      return;
    }
    if (tid == 0) cand[c] = bi;
    rescan = my_i == bi;  // a database index stands in one slot only: its owner retires it
    if (rescan) pd[my_slot] = -1.0f;
    __syncthreads();  // (block_argmin's scratch is read above and written again in the next round)
  }
}

__global__ __launch_bounds__(SC_BLOCK) void k_scq_detect(ScParams P, const double* __restrict__ desc, const double* __restrict__ pos,
                                                         const double* __restrict__ dist, const double* __restrict__ q_desc,
                                                         const double* __restrict__ q_pos, const double* __restrict__ q_dist,
                                                         const int32_t* __restrict__ cand_in, ScCandidate* __restrict__ records, int staged,
                                                         int prior) {
  const int q = blockIdx.x, c_only = blockIdx.y, tid = threadIdx.x;
  const int R = P.R, S = P.S;
  ScCandidate* rec = records + (size_t)q * gridDim.y + c_only;
  const int ci = cand_in[(size_t)q * gridDim.y + c_only];  // uniform
  if (ci < 0) {  // a rank beyond the query's candidates: k_scq_pick says so
    if (tid == 0) rec->idx = -1;
    return;
  }
  const int n_shift = 2 * P.radius + 1;
  const bool spread_shifts = n_shift <= S && n_shift * S <= SC_TERM_CAP;
  int argmin_shift;
  double min_sc;
  sc_descriptor_distance(P, q_desc + (size_t)q * R * S, desc + (size_t)ci * R * S, staged, spread_shifts, argmin_shift, min_sc);
  double cd = min_sc;
  if (prior) {  // the reference's formula with the query in the node's place
    const double odom_dist = sc_odom_term(P, q_pos[2 * (size_t)q], q_pos[2 * (size_t)q + 1], q_dist[q], pos[2 * (size_t)ci], pos[2 * (size_t)ci + 1], dist[ci]);
    cd = min_sc + odom_dist * R * P.odom_weight;
  }
  if (tid == 0) {
    rec->cd = cd;
    rec->shift = argmin_shift;
    rec->idx = ci;
  }
}

// the candidates of a query in rank order: the smallest distance wins, the first one on ties (:318-327); and what each was
__global__ __launch_bounds__(64) void k_scq_pick(ScParams P, int n_queries, int n_cand, const ScCandidate* __restrict__ records,
                                                 int32_t* __restrict__ loop_id, float* __restrict__ yaw, double* __restrict__ min_dist_out,
                                                 int32_t* __restrict__ cand_id, float* __restrict__ cand_yaw, double* __restrict__ cand_dist) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_queries) return;
  double min_d = 10000000;
  int nn_align = 0, nn_idx = 0;
  bool present = true;
  for (int c = 0; c < n_cand; ++c) {
    const ScCandidate r = records[(size_t)q * n_cand + c];
    present = present && r.idx >= 0;  // (ranks beyond the query's candidates: their records hold nothing else)
    if (present && r.cd < min_d) {
      min_d = r.cd;
      nn_align = r.shift;
      nn_idx = r.idx;
    }
    const size_t o = (size_t)q * n_cand + c;
    if (cand_id) cand_id[o] = present ? r.idx : -1;
    if (cand_yaw) cand_yaw[o] = present ? sc_shift_yaw(r.shift, P.S) : 0.0f;
    if (cand_dist) cand_dist[o] = present ? r.cd : 10000000;
  }
  if (loop_id) loop_id[q] = min_d < P.dist_thresh ? nn_idx : -1;
  if (yaw) yaw[q] = sc_shift_yaw(nn_align, P.S);
  if (min_dist_out) min_dist_out[q] = min_d;
}

struct QueryWs {
  ScCandidate* records;
  int32_t *cand, *part_i;
  float* part_d;
  size_t bytes;
};

QueryWs query_ws(void* base, int n_queries, int n_db, int n_cand) {
  const size_t q = n_queries > 0 ? n_queries : 1, c = n_cand < 1 ? 1 : (n_cand > SC_MAX_CAND ? SC_MAX_CAND : n_cand);
  const size_t chunks = n_db > 0 ? ((size_t)n_db + SCQ_CHUNK - 1) / SCQ_CHUNK : 1;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  char* p = static_cast<char*>(base);
  QueryWs w;
  size_t off = 0;
  w.records = reinterpret_cast<ScCandidate*>(p + off);
  off += up(q * c * sizeof(ScCandidate));
  w.cand = reinterpret_cast<int32_t*>(p + off);
  off += up(q * c * sizeof(int32_t));
  w.part_d = reinterpret_cast<float*>(p + off);
  off += up(q * chunks * c * sizeof(float));
  w.part_i = reinterpret_cast<int32_t*>(p + off);
  off += up(q * chunks * c * sizeof(int32_t));
  w.bytes = off;
  return w;
}

}  // namespace

// records | candidate indices | the chunks' partial lists: distances, indices
size_t sc_query_ws_bytes(int n_queries, int n_db, int n_cand) { return query_ws(nullptr, n_queries, n_db, n_cand).bytes; }

int launch_sc_query(randt_ctx* ctx, const randt_sc_params* p, const double* d_desc, const double* d_ring_keys, const double* d_pos,
                    const double* d_dist, int n_db, const double* d_q_desc, const double* d_q_ring_keys, const double* d_q_pos,
                    const double* d_q_dist, int n_queries, void* d_ws, int32_t* d_loop_id, float* d_yaw, double* d_min_dist,
                    int32_t* d_cand_id, float* d_cand_yaw, double* d_cand_dist) {
  if (n_queries <= 0) return RANDT_OK;
  if (p->num_ring < 1 || p->num_ring > SC_MAX_RING || p->num_sector < 1 || p->num_sector > SC_MAX_SECTOR || p->num_candidates < 1 ||
      p->num_candidates > SC_MAX_CAND)
    return randt_set_error(ctx, RANDT_ERR_UNSUPPORTED, "scan context: num_ring <= 64, num_sector <= 128, num_candidates <= 32", hipSuccess);
  const int n_chunks = n_db > 0 ? (int)(((size_t)n_db + SCQ_CHUNK - 1) / SCQ_CHUNK) : 0;
  if (n_chunks > 65535 || n_queries > 65535)
    return randt_set_error(ctx, RANDT_ERR_UNSUPPORTED, "scan context query: more than 65535 chunks of the database, or queries, in one call", hipSuccess);
  size_t lds = 2 * sizeof(double) * (size_t)p->num_ring * p->num_sector;
  const int staged = lds + 40 * 1024 <= (size_t)ctx->lds_limit ? 1 : 0;  // launch_sc_detect's rule (the static arrays take 37 KB)
  if (!staged) lds = 0;
  RANDT_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_scq_detect), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const size_t lds_keys = sizeof(float) * SCQ_CHUNK * (size_t)(p->num_ring | 1);  // k_scq_chunk's keys (133 KB at 64 rings; its static arrays take 2.3 KB)
  if (lds_keys + 4 * 1024 > (size_t)ctx->lds_limit)
    return randt_set_error(ctx, RANDT_ERR_UNSUPPORTED, "scan context query: the ring keys of one chunk do not fit the LDS", hipSuccess);
  RANDT_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_scq_chunk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_keys));
  const QueryWs w = query_ws(d_ws, n_queries, n_db, p->num_candidates);
  const ScParams P = to_dev(p);
  const int prior = d_q_pos && d_q_dist && d_pos && d_dist ? 1 : 0;
  if (n_chunks > 0)
    hipLaunchKernelGGL(k_scq_chunk, dim3(n_queries, n_chunks), dim3(SC_BLOCK), lds_keys, ctx->stream, P, d_ring_keys, n_db, d_q_ring_keys, w.part_d, w.part_i);
  hipLaunchKernelGGL(k_scq_merge, dim3(n_queries), dim3(SC_BLOCK), 0, ctx->stream, P, n_chunks * p->num_candidates, w.part_d, w.part_i, w.cand);
  hipLaunchKernelGGL(k_scq_detect, dim3(n_queries, p->num_candidates), dim3(SC_BLOCK), lds, ctx->stream, P, d_desc, d_pos, d_dist, d_q_desc, d_q_pos,
                     d_q_dist, w.cand, w.records, staged, prior);
  hipLaunchKernelGGL(k_scq_pick, dim3((n_queries + 63) / 64), dim3(64), 0, ctx->stream, P, n_queries, p->num_candidates, w.records, d_loop_id, d_yaw,
                     d_min_dist, d_cand_id, d_cand_yaw, d_cand_dist);
  RANDT_HIP_CHECK(ctx, hipGetLastError());
  return RANDT_OK;
}
