// bpr_rerank.hip — fused candidate re-ranking of libbprcore: every row (a user and a list of candidate items) is
// scored on ITS candidates only and its k best come back, with no [nnz, d] gather buffer and no sweep of the item
// table (bpr_rerank_rows / bpr_rerank_layout; the definition is the comment in include/bprcore.h).
//
// The reference has no candidate path: it ranks through full logits (example.py:195-230), which bpr_topk_rows
// replaces for "the k best of the catalogue".  This is that ranking restricted to a given list — availability
// filters, second-stage re-ranking, the 1 + N sampled-negative protocol, explicit (user, item) pairs.
//
// Unlike k_topk / k_rank / k_neighbors this is a GATHER: nnz * d * 4 bytes against 2 * nnz * d flops, memory-bound
// like the training kernels, so there is no MFMA here.  A team of threads (a wave, or the workgroup: the plan,
// bpr_rerank_plan.h) owns a row and walks its list a tile at a time:
//   (E) eligibility: a thread per candidate — 0 < id < I and not in the user's sorted seen row (one binary search
//       per candidate, all lanes searching at once in a row that stays in L2) — BEFORE anything of Q is read: an
//       ineligible candidate costs no table traffic, and its score is -inf;
//   (S) the tile's item rows travel global -> registers -> LDS RERANK_KC features at a time (8 lanes read 128
//       consecutive bytes of one row; padded [tile][RERANK_LD] chunks as in k_topk), the next chunk in flight while
//       the current one is multiplied; P[u] sits whole in LDS, read as a broadcast;
//   (M) ONE thread owns ONE candidate's accumulator: no cross-lane reduction;
//   (A)(B)(C) selection, k_topk's scheme per row: tau = the k-th best at the last compaction; (A) count what beats
//       it, (B) compact the buffer of k + tile entries when they might not fit, (C) append what beats the tightened
//       tau.  Nothing is dropped whatever the data.
//
// Numerics.  s(u, i) is bpr_topk_rows' score bit for bit: one fp32 accumulator from +0 through k_topk's chain in
// one thread (fma_chain8, bpr_topk_shared.h, which states the order), every chunk of 32 run to its end with zeros
// staged past d on both sides, then the bias as one fp32 add.
//
// Order.  Duplicates make (score desc, id asc) a preorder, and rank counting needs distinct ranks, so the order here
// has a third key: the candidate's position in its list.  Two entries that differ only in position are the same
// (score, id) pair to the caller, so the OUTPUT is a function of the multiset of candidates alone: not of their
// order, of the row's place, of the team or of the grid.  Because of the third key Cand, better and compact_row are
// this file's own (DESIGN 4.10 records why compact_row is not the shared one); the rest is bpr_topk_shared.h's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_rerank_plan.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {
namespace rr {

struct Cand {
  float s;
  int32_t i;
  uint32_t p;  // position in the row's list (its low 32 bits): only ever separates copies of one (s, i)
};

struct RerankArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* users;
  int64_t n;
  const int64_t* cptr;    // [n + 1], or nullptr: every row has the `shared` candidates of citems[0 ..)
  const int32_t* citems;
  int64_t shared;
  const int64_t* indptr;  // seen CSR, or nullptr
  const int32_t* indices;
  int k;
  float* cand_scores;     // aligned with the candidates ([n, shared] in shared mode), or nullptr
  int32_t* out_items;     // [n, k]
  float* out_scores;      // [n, k]
};

// the order of the result: score descending, ties by ascending item id, copies by position (never true for NaN)
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  return a.s > b.s || (a.s == b.s && (a.i < b.i || (a.i == b.i && a.p < b.p)));
}

// One wave: the c <= 64 * QN candidates of a row -> its min(c, k) best, sorted, in buf[0 ..); tau and count follow
// (k >= 1).  Every lane of the wave calls it with the same arguments.
template <int QN>
__device__ __forceinline__ void compact_row(Cand* buf, int c, int k, int lane, Cand* tau, int* cnt) {
  Cand e[QN];
  int rank[QN];
#pragma unroll
  for (int q = 0; q < QN; ++q) {
    const int idx = lane + 64 * q;
    e[q] = idx < c ? buf[idx] : Cand{0.0f, 0, 0u};
    rank[q] = 0;
  }
  for (int j = 0; j < c; ++j) {
    const Cand o = buf[j];
#pragma unroll
    for (int q = 0; q < QN; ++q) rank[q] += better(o, e[q]) ? 1 : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < QN; ++q) {
    if (lane + 64 * q < c && rank[q] < k) {
      buf[rank[q]] = e[q];
      if (rank[q] == k - 1) *tau = e[q];
    }
  }
  if (lane == 0) *cnt = c < k ? c : k;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the team's barrier: the workgroup's, or (a wave is its own team, and the waves of a workgroup walk rows of
// different lengths) the wave's own LDS order
template <int TEAM>
__device__ __forceinline__ void team_sync() {
  if (TEAM == RERANK_THREADS) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// VEC: d % 4 == 0 and a 16-byte aligned item table (16-byte global loads); else element loads.  TEAM: threads that
// own a row, 64 or 256; the tile is TEAM candidates, one chain per thread.
template <bool VEC, int TEAM>
__global__ __launch_bounds__(RERANK_THREADS) void k_rerank(const RerankArgs a, const unsigned team_lds) {
  constexpr int TILE = TEAM, KC = RERANK_KC, LD = RERANK_LD;
  constexpr int TEAMS = RERANK_THREADS / TEAM;  // rows of a workgroup
  constexpr int NF = TILE * (KC / 4) / TEAM;    // 16-byte pieces of a chunk a thread moves: 8
  constexpr int QN = (TOPK_MAX + TILE) / 64;    // entries of the fullest buffer a lane ranks
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x % TEAM, team = threadIdx.x / TEAM, lane = threadIdx.x & 63;
  const int dpad = (a.d + KC - 1) / KC * KC, nch = dpad / KC, cap = a.k + TILE;
  unsigned char* const base = smem + (size_t)team * team_lds;
  float* const sQ = reinterpret_cast<float*>(base);       // [TILE][LD]
  float* const sP = sQ + TILE * LD;                       // [dpad]
  int32_t* const sItem = reinterpret_cast<int32_t*>(sP + dpad);  // [TILE]: the eligible id, or -1
  Cand* const sBuf = reinterpret_cast<Cand*>(sItem + TILE);      // [cap]
  Cand* const sTau = sBuf + cap;
  int* const sCnt = reinterpret_cast<int*>(sTau + 1);
  int* const sNeed = sCnt + 1;
  const bool has_bias = a.bias != nullptr, select = a.k > 0;

  for (int64_t row = (int64_t)blockIdx.x * TEAMS + team; row < a.n; row += (int64_t)gridDim.x * TEAMS) {
    // ---- the row: every thread of the team reads the same few words (one broadcast load each)
    const int u = a.users[row];
    int64_t clo = 0, clen = a.shared, obase = row * a.shared;
    if (a.cptr != nullptr) {
      clo = a.cptr[row];
      clen = a.cptr[row + 1] - clo;
      obase = clo;
    }
    int64_t slo = 0, slen = 0;
    if (a.indptr != nullptr) {
      slo = a.indptr[u];
      slen = a.indptr[u + 1] - slo;
    }
    const int32_t* const seen = a.indices + slo;
    const float* const prow = a.P + (int64_t)u * a.d;
    for (int f = tid; f < dpad; f += TEAM) sP[f] = f < a.d ? prow[f] : 0.f;
    if (tid == 0) {
      *sCnt = 0;
      *sNeed = 0;
      *sTau = Cand{-INFINITY, INT_MAX, UINT_MAX};  // nothing kept yet: everything beats tau
    }
    team_sync<TEAM>();

    for (int64_t t0 = 0; t0 < clen; t0 += TILE) {
      // (E) eligibility, before any row of Q is touched
      const int64_t pos = t0 + tid;
      int item = -1;
      if (pos < clen) {
        const int c = a.citems[clo + pos];
        if (c > 0 && c < a.I && !in_sorted(seen, slen, c)) item = c;
        else if (a.cand_scores != nullptr) a.cand_scores[obase + pos] = -INFINITY;
      }
      sItem[tid] = item;
      const float bv = has_bias && item >= 0 ? a.bias[item] : 0.f;
      team_sync<TEAM>();

      // (S) + (M): piece f of a chunk is features 4 (f & 7) .. + 3 of the tile's candidate f >> 3
      float4 qreg[NF];
      auto fetch = [&](int c) {
        const int kc = c * KC;
#pragma unroll
        for (int m = 0; m < NF; ++m) {
          const int f = tid + TEAM * m, it = sItem[f >> 3];
          qreg[m] = it >= 0 ? load4<VEC>(a.Q + (int64_t)it * a.d, kc + 4 * (f & 7), a.d)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      };
      fetch(0);
      float acc = 0.f;
      const float* const q = sQ + tid * LD;
      for (int c = 0; c < nch; ++c) {
        BPR_STASH_CHUNK(sQ, qreg, NF, tid, TEAM);
        team_sync<TEAM>();
        if (c + 1 < nch) fetch(c + 1);
        const float* const p = sP + c * KC;
#pragma unroll
        for (int blk = 0; blk < KC / 8; ++blk) {
          const float4 q0 = *reinterpret_cast<const float4*>(q + 8 * blk);
          const float4 q1 = *reinterpret_cast<const float4*>(q + 8 * blk + 4);
          const float4 p0 = *reinterpret_cast<const float4*>(p + 8 * blk);
          const float4 p1 = *reinterpret_cast<const float4*>(p + 8 * blk + 4);
          acc = fma_chain8(q0, q1, p0, p1, acc);
        }
        team_sync<TEAM>();  // the chunk is read: the next one may be written over it
      }
      const Cand me = {has_bias ? acc + bv : acc, item, (uint32_t)pos};
      if (item >= 0 && a.cand_scores != nullptr) a.cand_scores[obase + pos] = me.s;
      if (!select) continue;

      // (A) how many of the tile beat the row's threshold
      bool beats = item >= 0 && better(me, *sTau);
      if (beats) atomicAdd(sNeed, 1);
      team_sync<TEAM>();
      // (B) a buffer that might not take them all: down to the k best (then count <= k, and a tile adds <= TILE)
      const int have = min(*sCnt, cap);
      if (have + *sNeed > cap && tid < 64) compact_row<QN>(sBuf, have, a.k, lane, sTau, sCnt);
      team_sync<TEAM>();
      // (C) append what still beats the threshold
      if (tid == 0) *sNeed = 0;
      if (beats && better(me, *sTau)) {
        const int at = atomicAdd(sCnt, 1);
        if (at < cap) sBuf[at] = me;
      }
      team_sync<TEAM>();
    }

    // ---- the row's result: sorted, padded with (-inf, -1)
    if (select) {
      if (tid < 64) {
        const int c = min(*sCnt, cap);
        if (c > 0) compact_row<QN>(sBuf, c, a.k, lane, sTau, sCnt);
        const int have = c < a.k ? c : a.k;
        for (int j = lane; j < a.k; j += 64) {
          const bool live = j < have;
          a.out_scores[row * a.k + j] = live ? sBuf[j].s : -INFINITY;
          a.out_items[row * a.k + j] = live ? sBuf[j].i : -1;
        }
      }
      team_sync<TEAM>();  // the buffer is read: the next row may reset it
    }
  }
}

static int check_shape(const char* who, int64_t n, int32_t d, int32_t k, int64_t row_len, int32_t layout) {
  if (n < 0) return fail(BPR_ERR_INVALID, std::string(who) + ": n must be >= 0");
  if (d < 1 || d > RERANK_DMAX) return fail(BPR_ERR_INVALID, std::string(who) + ": d must be in [1, 1024]");
  if (k < 0 || k > TOPK_MAX)
    return fail(BPR_ERR_INVALID, std::string(who) + ": k must be in [0, " + std::to_string(TOPK_MAX) + "]");
  if (row_len < 0) return fail(BPR_ERR_INVALID, std::string(who) + ": the list length must be >= 0");
  if (layout < 0 || layout > RERANK_LAYOUTS)
    return fail(BPR_ERR_INVALID, std::string(who) + ": layout must be 0 (choose), 1 (wave per row) or 2 (workgroup "
                                                    "per row)");
  return BPR_OK;
}

}  // namespace rr
}  // namespace bpr

extern "C" int bpr_rerank_layout(int64_t n, int32_t d, int32_t k, int64_t row_len, int32_t layout,
                                 int32_t* layout_host, int32_t* tile_host) {
  using namespace bpr;
  if (layout_host == nullptr || tile_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_rerank_layout: layout_host or tile_host is NULL");
  if (int rc = rr::check_shape("bpr_rerank_layout", n, d, k, row_len, layout)) return rc;
  const RerankPlan p = plan_rerank(n, d, k, row_len, layout);
  *layout_host = p.layout;
  *tile_host = p.tile;
  return BPR_OK;
}

extern "C" int bpr_rerank_rows(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                               const int32_t* users, int64_t n, const int64_t* cand_indptr,
                               const int32_t* cand_items, int64_t shared_len, const int64_t* seen_indptr,
                               const int32_t* seen_indices, int32_t k, int32_t layout, float* cand_scores_out,
                               int32_t* items_out, float* scores_out, void* hip_stream) {
  using namespace bpr;
  using namespace bpr::rr;
  if (int rc = check_shape("bpr_rerank_rows", n, d, k, shared_len, layout)) return rc;
  if (I < 1 || I >= ((int64_t)1 << 31)) return fail(BPR_ERR_INVALID, "bpr_rerank_rows: I must be in [1, 2^31)");
  if (k == 0 && cand_scores_out == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_rerank_rows: k == 0 asks for the candidate scores only: cand_scores_out is NULL");
  if ((seen_indptr == nullptr) != (seen_indices == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_rerank_rows: seen_indptr and seen_indices go together");
  if (n == 0) return BPR_OK;
  if (!P || !Q || !users) return fail(BPR_ERR_INVALID, "bpr_rerank_rows: P, Q or users is NULL");
  if (cand_items == nullptr && (cand_indptr != nullptr || shared_len > 0))
    return fail(BPR_ERR_INVALID, "bpr_rerank_rows: cand_items is NULL");
  if (k > 0 && (!items_out || !scores_out))
    return fail(BPR_ERR_INVALID, "bpr_rerank_rows: items_out or scores_out is NULL");

  const RerankPlan p = plan_rerank(n, d, k, shared_len, layout);
  RerankArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.users = users; a.n = n;
  a.cptr = cand_indptr; a.citems = cand_items; a.shared = cand_indptr != nullptr ? 0 : shared_len;
  a.indptr = seen_indptr; a.indices = seen_indices; a.k = k;
  a.cand_scores = cand_scores_out; a.out_items = items_out; a.out_scores = scores_out;
  hipStream_t stream = (hipStream_t)hip_stream;
  const bool vec = vec_path(d, Q);
  const auto kernel = p.layout == RERANK_WAVE
                          ? (vec ? k_rerank<true, 64> : k_rerank<false, 64>)
                          : (vec ? k_rerank<true, RERANK_THREADS> : k_rerank<false, RERANK_THREADS>);
  return launch_kernel(kernel, 0, dim3((unsigned)p.grid), dim3(RERANK_THREADS), p.lds, stream, a,
                       (unsigned)p.team_lds);
}

// Test hook, not API (tests/test_rerank_cpu.py sets its signature): the plan of a shape.  in = {n, d, k, row_len,
// layout}; out = {layout, tile, rows_per_group, cap, groups, grid, team_lds, lds, lds_limit, wave_max_len, grid_max,
// wave_mid_len, wave_mid_rows, wave_any_rows}.
// Needs no GPU.
extern "C" int bpr_test_rerank_plan(const int64_t* in, int64_t* out) {
  using namespace bpr;
  if (int rc = rr::check_shape("bpr_test_rerank_plan", in[0], (int32_t)in[1], (int32_t)in[2], in[3], (int32_t)in[4]))
    return rc;
  const RerankPlan p = plan_rerank(in[0], (int)in[1], (int)in[2], in[3], (int)in[4]);
  const int64_t v[] = {p.layout, p.tile, p.rows_per_group, p.cap, p.groups, p.grid, (int64_t)p.team_lds,
                       (int64_t)p.lds, (int64_t)RERANK_LDS_LIMIT, RERANK_WAVE_MAX_LEN, RERANK_GRID_MAX,
                       RERANK_WAVE_MID_LEN, RERANK_WAVE_MID_ROWS, RERANK_WAVE_ANY_ROWS};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}
