// bpr_neighbors.hip — fused neighbour search of libbprcore: the k rows of a table T most similar to each of a list
// of query rows X[rows[r]], by dot product or cosine, with no [n, N] score matrix anywhere (bpr_neighbors_rows /
// bpr_neighbors_workspace / bpr_neighbors_slices; the definition is the comment in include/bprcore.h).
//
// The kernel has k_topk's structure (bpr_topk.hip, which explains it at length): 256 threads own 64 queries and
// stream the table past them 128 rows x 32 features at a time through LDS into exact f32 MFMA accumulators
// (v_mfma_f32_32x32x2_f32: table rows on the A side, queries on the B side, so a lane's 16 results are 16 table
// rows of ONE query); every query keeps in LDS a threshold tau = its k-th best at the last compaction, a buffer of
// k + 128 candidates and a count; after a table tile (A) every lane counts its eligible scores that beat tau, (B) a
// query whose buffer could overflow is compacted by one wave to its k best, sorted, (C) what still beats the
// tightened tau is appended.  The dot product is k_topk's fmaf chain, bit for bit: staging, the chain, Cand, better,
// compact_row and step (B) are the same code (bpr_topk_shared.h), and the slices are merged by k_topk_merge.
//
// What differs from k_topk:
//   - queries are gathered through `rows` from X, which need not be the table;
//   - the per-query LDS state carries the excluded id and the query's reciprocal norm instead of a seen row;
//   - under the cosine metric the reciprocal norms of the table tile travel with the tile's first chunk (global ->
//     register -> LDS), and the two multiplications are applied to the accumulator before the tau compare;
//   - eligibility is two integer compares and one float compare on values the lane already holds, so it is part
//     of (A)'s mask: (C) touches no global memory, where k_topk's (C) runs a binary search in the seen CSR per
//     candidate.  profiles/similar_probe.txt measures what that is worth.
//
// Cosine pre-pass (k_neighbors_norms): one thread per row folds v_f * v_f into ONE fmaf chain from 0 over the
// features in the dot product's own order (fma_chain8, bpr_topk_shared.h), so ss(v) == dot(v, v) bit for
// bit and a row meets its own copy at (ss * rn) * rn, six roundings from 1; rn = 1 / sqrt(ss), both correctly
// rounded, is stored if ss > 0, the marker -1 otherwise (a zero row, or one with a NaN): such a table row is never
// returned, such a query gets a padded row.  An ss that overflowed is +inf > 0: rn = +0, the row stays eligible and
// its scores are +-0 or (inf * 0) NaN, which is never returned (tests/test_gpu_chain.py, class d).  The norms of the N
// table rows and the n queries are written on every call.
// Correct rounding is spelt sqrtf and `/` here, and the Makefile pins -fhip-fp32-correctly-rounded-divide-sqrt for
// this object: HIP's __fsqrt_rn is the hardware's approximate square root (1 ulp) unless the headers are built
// with OCML_BASIC_ROUNDED_OPERATIONS, whose __ocml_sqrt_rte_f32 / __ocml_div_rte_f32 the device library of this
// toolchain does not carry, and its __fdiv_rn is `/`.  tests/test_gpu_similar.py holds the bits to numpy's IEEE
// float32, so a build that rounds otherwise fails there.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_item_filter.h"
#include "bpr_neighbors_plan.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {
namespace nbr {

struct NeighborsArgs {
  const float* X;
  const float* T;
  int64_t N;
  int d;
  const int32_t* rows;
  int64_t n;
  const int32_t* exclude;  // [n] or nullptr
  int first;
  const float* rn_t;  // [N], cosine only
  const float* rn_x;  // [n], cosine only
  int k, slices;
  int64_t tiles;
  float* out_scores;  // [n, slices, k]
  int32_t* out_ids;   // [n, slices, k]
};

// rn of the N table rows, then of the n queries: one thread per row (the order of the chain: bpr_topk_shared.h;
// features past d are read as zeros, and fmaf(0, 0, ss) == ss)
template <bool VEC>
__global__ __launch_bounds__(256) void k_neighbors_norms(const float* __restrict__ T, int64_t N,
                                                         const float* __restrict__ X,
                                                         const int32_t* __restrict__ rows, int64_t n, int d,
                                                         float* __restrict__ rn_t, float* __restrict__ rn_x) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float* src;
  float* dst;
  if (g < N) {
    src = T + g * d;
    dst = rn_t + g;
  } else if (g - N < n) {
    src = X + (int64_t)rows[g - N] * d;
    dst = rn_x + (g - N);
  } else {
    return;
  }
  float ss = 0.f;
  for (int f = 0; f < d; f += 8) {
    const float4 lo = load4<VEC>(src, f, d), hi = load4<VEC>(src, f + 4, d);
    ss = fma_chain8(lo, hi, lo, hi, ss);
  }
  *dst = ss > 0.f ? 1.0f / sqrtf(ss) : -1.0f;  // (correctly rounded: the head of this file)
}

// VEC: d % 4 == 0 and 16-byte aligned tables (16-byte global loads); else element loads.  COS: cosine metric.
// FILT: a filter over the N table rows (bpr_item_filter.h, with `first` as its lower bound) lies behind the
// arguments: a row whose bit is clear is not eligible, and the loop walks the slice's non-empty tiles only.  Without
// it the kernel is what it was before there were filters.
template <bool VEC, bool COS, bool FILT>
__global__ __launch_bounds__(256) void k_neighbors(const MaybeFiltered<FILT, NeighborsArgs> a) {
  constexpr int TU = TOPK_TU, TI = TOPK_TI, LD = TOPK_LD;
  extern __shared__ __align__(16) unsigned char smem[];
  const int cap = a.k + TI;
  float* const sT = reinterpret_cast<float*>(smem);          // [TI][LD]
  float* const sX = sT + TI * LD;                            // [TU][LD]
  float* const sRnT = sX + TU * LD;                          // [TI]
  Cand* const sBuf = reinterpret_cast<Cand*>(sRnT + TI);     // [TU][cap]
  Cand* const sTau = sBuf + TU * cap;                        // [TU]
  int* const sCnt = reinterpret_cast<int*>(sTau + TU);
  int* const sNeed = sCnt + TU;
  int* const sRow = sNeed + TU;
  int* const sExcl = sRow + TU;
  float* const sRnX = reinterpret_cast<float*>(sExcl + TU);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t u0 = (int64_t)blockIdx.x * TU;
  const int slice = blockIdx.y;
  const int64_t t0 = a.tiles * slice / a.slices, t1 = a.tiles * (slice + 1) / a.slices;

  if (tid < TU) {
    const int64_t q = u0 + tid;
    const bool live = q < a.n;
    const float rx = COS && live ? a.rn_x[q] : 1.0f;
    sRow[tid] = live ? a.rows[q] : -1;
    sExcl[tid] = live && a.exclude != nullptr ? a.exclude[q] : -1;
    sRnX[tid] = rx;
    sCnt[tid] = 0;
    sNeed[tid] = 0;
    // nothing kept yet: everything beats tau; a query past n, or (cosine) without a norm: nothing does
    sTau[tid] = live && rx >= 0.f ? Cand{-INFINITY, INT_MAX} : Cand{INFINITY, -1};
  }
  __syncthreads();

  // the walk (bpr_topk_shared.h).  FILT: the slice's non-empty tiles only.  Cosine: a tile's norms travel with its
  // first chunk (read in (A) of this tile only, which a barrier separates from the next tile's first stash).
  float rnreg = 0.f;
  auto fetch_norms = [&](int64_t t, int c) {
    if (COS && c == 0 && tid < TI) {
      const int64_t j = t * TI + tid;
      rnreg = j < a.N ? a.rn_t[j] : -1.0f;
    }
  };
  auto stash_norms = [&](int64_t, int c) {
    if (COS && c == 0 && tid < TI) sRnT[tid] = rnreg;
  };
  auto tile_from = [&](int64_t t) -> int64_t {
    if constexpr (FILT) return filter_next_tile_from(a.filter, a.N, t, t1, a.first);
    else return t;
  };
  const table_tiles table = {a.N};
  BPR_WALK_LANE(a.d, sT, sX);
  BPR_WALK_TILES_BEGIN(VEC, FILT, tile_from(t0), t1, table, a.T, a.X, a.d, sRow, sT, sX, tile_from, fetch_norms,
                       stash_norms)

    // ---- epilogue of the tile: register q of the lane is table row jbase + (q & 3) + 8 (q >> 2) of queries r, 32 + r
    const int64_t jbase = t * TI + 32 * w + 4 * h;
    // (A) the eligible scores that beat the query's threshold; under cosine the accumulators become the scores
    // the wave's word of the filter: bit b is table row t * TI + 32 w + b
    uint32_t fw = 0;
    if constexpr (FILT) fw = filter_wave_word_from(a.filter, a.N, t, __builtin_amdgcn_readfirstlane(w), a.first);
    unsigned m0 = 0, m1 = 0;
    {
      const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
      const int ex0 = sExcl[r], ex1 = sExcl[32 + r];
      const float rx0 = sRnX[r], rx1 = sRnX[32 + r];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int jl = 32 * w + 4 * h + (q & 3) + 8 * (q >> 2);
        const int64_t j = t * TI + jl;
        bool ok = j >= a.first && j < a.N && (!FILT || ((fw >> (jl & 31)) & 1u));
        if (COS) {
          const float rt = sRnT[jl];
          ok = ok && rt >= 0.f;
          acc0[q] = __fmul_rn(__fmul_rn(acc0[q], rt), rx0);
          acc1[q] = __fmul_rn(__fmul_rn(acc1[q], rt), rx1);
        }
        if (ok && (int)j != ex0 && better(acc0[q], (int)j, tau0.s, tau0.i)) m0 |= 1u << q;
        if (ok && (int)j != ex1 && better(acc1[q], (int)j, tau1.s, tau1.i)) m1 |= 1u << q;
      }
      if (m0) atomicAdd(&sNeed[r], __popc(m0));
      if (m1) atomicAdd(&sNeed[32 + r], __popc(m1));
    }
    __syncthreads();
    // (B) queries whose buffer might not take them all are compacted, which tightens tau
    compact_overflowing_rows(sBuf, sCnt, sNeed, sTau, cap, a.k, w, lane);
    __syncthreads();
    // (C) append what still beats the threshold: no global memory is touched
    if (tid < TU) sNeed[tid] = 0;
    if (m0 | m1) {
      const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = (int)(jbase + (q & 3) + 8 * (q >> 2));
        if (((m0 >> q) & 1u) && better(acc0[q], j, tau0.s, tau0.i)) {
          const int pos = atomicAdd(&sCnt[r], 1);
          if (pos < cap) sBuf[r * cap + pos] = Cand{acc0[q], j};
        }
        if (((m1 >> q) & 1u) && better(acc1[q], j, tau1.s, tau1.i)) {
          const int pos = atomicAdd(&sCnt[32 + r], 1);
          if (pos < cap) sBuf[(32 + r) * cap + pos] = Cand{acc1[q], j};
        }
      }
    }
  BPR_WALK_TILES_END
  __syncthreads();

  // ---- the slice's result: every query sorted, padded with (-inf, -1)
  for (int row = w; row < TU; row += 4) {
    if (u0 + row >= a.n) break;
    const int c = min(sCnt[row], cap);
    Cand* const buf = sBuf + row * cap;
    if (c > 0) compact_row(buf, c, a.k, lane, &sTau[row], &sCnt[row]);
    const int have = c < a.k ? c : a.k;
    const int64_t out = ((u0 + row) * a.slices + slice) * a.k;
    for (int j = lane; j < a.k; j += 64) {
      const Cand e = j < have ? buf[j] : Cand{-INFINITY, -1};
      a.out_scores[out + j] = e.s;
      a.out_ids[out + j] = e.i;
    }
  }
}

static int check_metric(const char* who, int32_t metric) {
  if (metric != NBR_DOT && metric != NBR_COSINE)
    return fail(BPR_ERR_INVALID, std::string(who) + ": metric must be BPR_SIM_DOT (0) or BPR_SIM_COSINE (1)");
  return BPR_OK;
}

}  // namespace nbr
}  // namespace bpr

extern "C" int bpr_neighbors_workspace(int64_t n, int64_t N, int32_t d, int32_t k, int32_t metric,
                                       int32_t item_slices, int64_t* bytes_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_neighbors_workspace", bytes_host, "bytes_host")) return rc;
  if (int rc = check_topk_shape("bpr_neighbors_workspace", n, N, d, k, TOPK_MAX, item_slices, "N")) return rc;
  if (int rc = nbr::check_metric("bpr_neighbors_workspace", metric)) return rc;
  *bytes_host = neighbors_workspace_bytes(n, N, k, metric, item_slices);
  return BPR_OK;
}

extern "C" int bpr_neighbors_slices(int64_t n, int64_t N, int32_t d, int32_t k, int32_t item_slices,
                                    int32_t* slices_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_neighbors_slices", slices_host, "slices_host")) return rc;
  if (int rc = check_topk_shape("bpr_neighbors_slices", n, N, d, k, TOPK_MAX, item_slices, "N")) return rc;
  *slices_host = plan_neighbors(n, N, k, NBR_DOT, item_slices).t.slices;
  return BPR_OK;
}

namespace bpr {
namespace nbr {
namespace {

// bpr_neighbors_rows (rows_suffix = "_rows", no filter) and bpr_neighbors_rows_filtered ("_rows_filtered"): one
// body, the messages under the entry point's own name.  The plan does not look at the filter.
int neighbors_rows(const char* rows_suffix, const float* X, const float* T, int64_t N, int32_t d, const int32_t* rows,
                   int64_t n, const int32_t* exclude, int32_t first, int32_t metric, const uint32_t* item_filter,
                   int32_t k, int32_t item_slices, void* workspace, int64_t workspace_bytes, int32_t* ids_out,
                   float* scores_out, void* hip_stream) {
  const std::string who = std::string("bpr_neighbors") + rows_suffix;
  if (int rc = check_topk_shape(who.c_str(), n, N, d, k, TOPK_MAX, item_slices, "N")) return rc;
  if (int rc = check_metric(who.c_str(), metric)) return rc;
  if (first < 0) return fail(BPR_ERR_INVALID, who + ": first must be >= 0");
  if (n > 0 && (!X || !T || !rows || !ids_out || !scores_out))
    return fail(BPR_ERR_INVALID, who + ": X, T, rows, ids_out or scores_out is NULL");
  if (int rc = check_item_filter(who.c_str(), item_filter)) return rc;
  const NeighborsPlan p = plan_neighbors(n, N, k, metric, item_slices);
  if (int rc = check_workspace("bpr_neighbors", workspace, workspace_bytes, p.ws_bytes, nullptr, false, rows_suffix))
    return rc;
  if (n == 0) return BPR_OK;

  hipStream_t stream = (hipStream_t)hip_stream;
  const int S = p.t.slices;
  NeighborsArgs a = {};
  a.X = X; a.T = T; a.N = N; a.d = d; a.rows = rows; a.n = n; a.exclude = exclude; a.first = first;
  a.k = k; a.slices = S; a.tiles = p.t.item_tiles;
  // workspace: the slices' partial scores, their ids, then (cosine) rn of the table rows and of the queries
  slice_outputs(workspace, n, S, k, scores_out, ids_out, &a.out_scores, &a.out_ids);
  const bool vec = vec_path(d, X, T), cosine = metric == NBR_COSINE;
  if (cosine) {
    float* rn_t = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + p.partial_bytes);
    float* rn_x = rn_t + N;
    a.rn_t = rn_t;
    a.rn_x = rn_x;
    const int64_t blocks = (N + n + 255) / 256;  // < 2^24
    if (int rc = launch_kernel(vec ? k_neighbors_norms<true> : k_neighbors_norms<false>, 0, dim3((unsigned)blocks),
                               dim3(256), 0, stream, T, N, X, rows, n, (int)d, rn_t, rn_x))
      return rc;
  }
  const dim3 grid((unsigned)p.t.user_tiles, (unsigned)S);
  if (item_filter != nullptr) {
    Filtered<NeighborsArgs> f = {};
    static_cast<NeighborsArgs&>(f) = a;
    f.filter = item_filter;
    const auto kernel = cosine ? (vec ? k_neighbors<true, true, true> : k_neighbors<false, true, true>)
                               : (vec ? k_neighbors<true, false, true> : k_neighbors<false, false, true>);
    if (int rc = launch_kernel(kernel, neighbors_lds_bytes(TOPK_MAX), grid, dim3(256), p.lds, stream, f)) return rc;
  } else {
    const auto kernel = cosine ? (vec ? k_neighbors<true, true, false> : k_neighbors<false, true, false>)
                               : (vec ? k_neighbors<true, false, false> : k_neighbors<false, false, false>);
    if (int rc = launch_kernel(kernel, neighbors_lds_bytes(TOPK_MAX), grid, dim3(256), p.lds, stream, a)) return rc;
  }
  return launch_topk_merge(a.out_scores, a.out_ids, n, S, k, p.t.merge_lds, scores_out, ids_out, stream);
}

}  // namespace
}  // namespace nbr
}  // namespace bpr

extern "C" int bpr_neighbors_rows(const float* X, const float* T, int64_t N, int32_t d, const int32_t* rows, int64_t n,
                                  const int32_t* exclude, int32_t first, int32_t metric, int32_t k,
                                  int32_t item_slices, void* workspace, int64_t workspace_bytes, int32_t* ids_out,
                                  float* scores_out, void* hip_stream) {
  return bpr::nbr::neighbors_rows("_rows", X, T, N, d, rows, n, exclude, first, metric, nullptr, k, item_slices,
                                  workspace, workspace_bytes, ids_out, scores_out, hip_stream);
}

extern "C" int bpr_neighbors_rows_filtered(const float* X, const float* T, int64_t N, int32_t d, const int32_t* rows,
                                           int64_t n, const int32_t* exclude, int32_t first, int32_t metric,
                                           const uint32_t* item_filter, int32_t k, int32_t item_slices,
                                           void* workspace, int64_t workspace_bytes, int32_t* ids_out,
                                           float* scores_out, void* hip_stream) {
  return bpr::nbr::neighbors_rows("_rows_filtered", X, T, N, d, rows, n, exclude, first, metric, item_filter, k,
                                  item_slices, workspace, workspace_bytes, ids_out, scores_out, hip_stream);
}

// Test hook, not API (tests/test_neighbors_cpu.py sets its signature): the plan of a shape.  in = {n, N, d, k,
// metric, item_slices, cus}; out = {slices, query_tiles, table_tiles, tile_queries, tile_rows, cap, lds, lds_limit,
// merge_lds, partial_bytes, norm_bytes, ws_bytes}; bounds[0 .. slices] = first table row of each slice, then N.
// Needs no GPU.
extern "C" int bpr_test_neighbors_plan(const int64_t* in, int64_t* out, int64_t* bounds) {
  using namespace bpr;
  if (int rc = check_topk_shape("bpr_test_neighbors_plan", in[0], in[1], (int32_t)in[2], (int32_t)in[3], TOPK_MAX,
                                (int32_t)in[5], "N"))
    return rc;
  if (int rc = nbr::check_metric("bpr_test_neighbors_plan", (int32_t)in[4])) return rc;
  const NeighborsPlan p = plan_neighbors(in[0], in[1], (int)in[3], (int)in[4], (int)in[5],
                                         in[6] > 0 ? (int)in[6] : TOPK_CUS);
  const int64_t v[] = {p.t.slices, p.t.user_tiles, p.t.item_tiles, TOPK_TU, TOPK_TI, p.t.cap, (int64_t)p.lds,
                       (int64_t)NBR_LDS_LIMIT, (int64_t)p.t.merge_lds, p.partial_bytes, p.norm_bytes, p.ws_bytes};
  memcpy(out, v, sizeof(v));
  slice_bounds(p.t, topk_slice_tile, TOPK_TI, in[1], bounds);
  return BPR_OK;
}
