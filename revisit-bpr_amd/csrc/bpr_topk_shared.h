// bpr_topk_shared.h — what the serving kernels have in common (k_topk, bpr_topk.hip; k_retrieve, bpr_retrieve.hip;
// k_sample, bpr_sample.hip; k_rank, bpr_rank.hip; k_neighbors, bpr_neighbors.hip; k_rerank, bpr_rerank.hip;
// k_diversify, bpr_diversify.hip), each piece defined once.  Device side: the guarded load of 4 features (load4), the
// registers -> LDS copy of a staged chunk (stash_piece, BPR_STASH_CHUNK), the dot product's chain as MFMAs and as fmaf
// (mfma_chunk2, mfma_block1, fma_chain8), the result order (Cand, better), rank-by-counting compaction of a candidate
// buffer (compact_row), the selection step k_topk and k_neighbors run alike (compact_overflowing_rows), the row
// prologue (BPR_STAGE_USER_ROW, BPR_OPEN_SELECTION_ROW) and the tile walk of the kernels that stream a whole table
// past 64 rows (BPR_WALK_TILES_BEGIN / _END: k_topk, k_retrieve, k_sample, k_neighbors).  Device code only: what the
// entry points' host sides share is bpr_serving_host.h.  What differs between the kernels — where a staged row comes
// from, eligibility, what a score becomes — stays in their files.
//
// The walk's contract.  The 256 threads hold chunk (t, c) — TOPK_KC features of the TOPK_TI table rows of tile t and
// of the TOPK_TU rows — in registers one step before it is multiplied: the first chunk of the first tile is asked for
// before the loop, and right after chunk (t, c) has been written to LDS the next one is asked for, (t, c + 1) or,
// behind a tile's last chunk, chunk 0 of the tile that is walked next (nothing behind the last tile), so that its
// global loads fly while the MFMAs of (t, c) run and, behind a tile's last chunk, while the tile's epilogue runs.
// Two barriers a chunk.  The one before the stash: every wave has read the chunk before out of LDS, and is through
// the epilogue of the tile before, so whatever that epilogue read beside the chunks (k_neighbors' norms) may be
// written again.  The one after it: the chunk is whole before any wave multiplies it.  With a filter the tile that is
// walked next is not t + 1 but the next non-empty one, a scan over the filter's words: it is found once a tile (tn),
// at the tile's head, and serves both the prefetch behind the last chunk and the loop's step; without a filter the
// loop must stay `for (t = t0; t < t1; ++t)` to the compiler, which is why the step is written as it is.
// k_rank walks the same way but keeps its own copy of the loop (bpr_rank.hip): on the macros, and on the prologue's,
// its instantiations came out reordered, two of them with other register counts (profiles/serving_walk_resources.md).
//
// Every piece here compiles to the instructions of the same statements written out in each kernel; the pieces that
// did not in any form tried are still in the kernels' files (profiles/topk_shared_resources.md and
// profiles/serving_walk_resources.md name them).  No division and no square root: the header means the same under the
// Makefile's two flag sets.  Not for the plan headers, which stay plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "bpr_topk_plan.h"

namespace bpr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- staging: a chunk is [rows][TOPK_LD] floats in LDS, TOPK_KC features of every row (zeros past d, and for a row
// that is not there), moved as 16-byte pieces: piece f is features 4 (f & 7) .. + 3 of row f >> 3.

// VEC: d % 4 == 0 and a 16-byte aligned table (one 16-byte global load); else element loads.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, int kk, int d) {
  if (VEC) return kk < d ? *reinterpret_cast<const float4*>(row + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = kk + 0 < d ? row[kk + 0] : 0.f;
  v.y = kk + 1 < d ? row[kk + 1] : 0.f;
  v.z = kk + 2 < d ? row[kk + 2] : 0.f;
  v.w = kk + 3 < d ? row[kk + 3] : 0.f;
  return v;
}

// registers -> LDS, one piece
__device__ __forceinline__ void stash_piece(float* s, const float4 v, int f) {
  *reinterpret_cast<float4*>(s + (f >> 3) * TOPK_LD + 4 * (f & 7)) = v;
}

// registers -> LDS, a chunk: thread TID of STRIDE holds pieces TID + STRIDE * m in the float4 REG[M].  A macro, as
// the skeleton of bpr_foldin_shared.h and for its reason: a function that takes the array (by reference or as a
// pointer) costs k_rerank up to 6 VGPRs and an occupancy step and reschedules the others
// (profiles/topk_shared_resources.md); expanded in place, the loop compiles to the parent's instructions.
#define BPR_STASH_CHUNK(S, REG, M, TID, STRIDE) \
  _Pragma("unroll") for (int m_ = 0; m_ < (M); ++m_) bpr::stash_piece((S), (REG)[m_], (TID) + (STRIDE) * m_)

// ---- the chain.  A score is ONE fp32 accumulator from +0 through one fmaf per feature, per 8 features in the order
// 0, 4, 1, 5, 2, 6, 3, 7: v_mfma_f32_32x32x2_f32 takes two features a step, one from each lane half, and a lane
// half reads 4 consecutive features of a staged row with one 16-byte LDS read, so the halves hold 0 .. 3 and 4 .. 7.
// Every chunk is run to its end over the staged zeros.  The order is a contract, not a detail: the kernels are held
// to each other bit for bit (rerank against bpr_topk_rows and bpr_rank_rows, the cosine norms against the dot
// product, diversify's Gram matrix against the scores), so a score's bits are the same wherever the pair falls —
// in a tile, a slice, a list, or another kernel.  Whoever changes the order changes it here, for all of them.
// The host statement of the contract is tests/chain_model.py (numpy, a correctly rounded fma, held to exact rational
// arithmetic by tests/test_chain_model_cpu.py); tests/test_gpu_chain.py holds every kernel's scores to its bits, so
// a change here that moves all kernels together is still seen.  That includes the values at the edge: subnormal
// products and sums are kept, by the MFMA as by fmaf (measured on gfx950: IEEE, bit for bit); a negative product that
// underflows onto the zero accumulator is -0 and the staged zeros after it make +0 of it (which is why a chunk is run
// to its end); 0 * inf over a staged zero is NaN, a NaN score is never `better` than anything and so never enters a
// buffer, and +-inf scores are ordered like any other — a real item at -inf beats the padding (-inf, -1) and
// k_retrieve's sort sentinel (-inf, INT_MAX) by its id.

// 8 features of one 32 x 32 tile: a, b are the lane's 4 staged features of its A-side and B-side row
__device__ __forceinline__ void mfma_block1(const float4 a, const float4 b, f32x16& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// One staged chunk of two tiles that share their A side: qa, pb0, pb1 point at the lane's row + 4 * (lane >> 5) of
// the A-side chunk and of the two B-side row blocks.  The two accumulators alternate, so that no MFMA waits for the
// one before it.
__device__ __forceinline__ void mfma_chunk2(const float* qa, const float* pb0, const float* pb1, f32x16& acc0,
                                            f32x16& acc1) {
#pragma unroll
  for (int blk = 0; blk < TOPK_KC / 8; ++blk) {
    const float4 a4 = *reinterpret_cast<const float4*>(qa + 8 * blk);
    const float4 b0 = *reinterpret_cast<const float4*>(pb0 + 8 * blk);
    const float4 b1 = *reinterpret_cast<const float4*>(pb1 + 8 * blk);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b0.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b0.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b0.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b1.w, acc1, 0, 0, 0);
  }
}

// the same 8 features in one thread: q0, p0 are features 0 .. 3 of the two rows, q1, p1 features 4 .. 7
__device__ __forceinline__ float fma_chain8(const float4 q0, const float4 q1, const float4 p0, const float4 p1,
                                            float acc) {
  acc = __fmaf_rn(q0.x, p0.x, acc);
  acc = __fmaf_rn(q1.x, p1.x, acc);
  acc = __fmaf_rn(q0.y, p0.y, acc);
  acc = __fmaf_rn(q1.y, p1.y, acc);
  acc = __fmaf_rn(q0.z, p0.z, acc);
  acc = __fmaf_rn(q1.z, p1.z, acc);
  acc = __fmaf_rn(q0.w, p0.w, acc);
  acc = __fmaf_rn(q1.w, p1.w, acc);
  return acc;
}

// ---- selection

struct Cand {
  float s;
  int32_t i;
};

// the order of the result: score descending, ties by ascending id (never true for a NaN score)
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// L: the type of the length (k_topk searches with 32-bit indices, k_rerank's rows may be longer)
template <typename L>
__device__ __forceinline__ bool in_sorted(const int32_t* __restrict__ v, L len, int item) {
  L lo = 0, hi = len;
  while (lo < hi) {
    const L mid = (lo + hi) >> 1;
    if (v[mid] < item) lo = mid + 1; else hi = mid;
  }
  return lo < len && v[lo] == item;
}

// One wave: the c <= k + TOPK_TI <= 256 candidates of a row -> its min(c, k) best, sorted, in buf[0 ..); tau and
// count follow.  Rank by counting: `better` is a strict total order on what a buffer holds (ids are distinct), so
// ranks are distinct.  Every lane of the wave calls it with the same arguments.  (k_rerank's order has a third key
// and its lanes rank more entries: its compact_row is its own, bpr_rerank.hip.)
__device__ __forceinline__ void compact_row(Cand* buf, int c, int k, int lane, Cand* tau, int* cnt) {
  Cand e[4];
  int rank[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = lane + 64 * q;
    e[q] = idx < c ? buf[idx] : Cand{0.0f, 0};
    rank[q] = 0;
  }
  for (int j = 0; j < c; ++j) {
    const Cand o = buf[j];
#pragma unroll
    for (int q = 0; q < 4; ++q) rank[q] += better(o.s, o.i, e[q].s, e[q].i) ? 1 : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (lane + 64 * q < c && rank[q] < k) {
      buf[rank[q]] = e[q];
      if (rank[q] == k - 1) *tau = e[q];
    }
  }
  if (lane == 0) *cnt = c < k ? c : k;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The TOPK_TU rows of a k_topk / k_neighbors workgroup keep [cap = k + TOPK_TI] candidates, a count, a threshold tau
// and `need`, how many scores of the current tile beat tau; wave w of the 4 owns rows w, w + 4, ...
// Step (B): rows whose buffer might not take the tile: down to the k best (then count <= k, and a tile adds <= TI).
__device__ __forceinline__ void compact_overflowing_rows(Cand* sBuf, int* sCnt, const int* sNeed, Cand* sTau, int cap,
                                                         int k, int w, int lane) {
  for (int row = w; row < TOPK_TU; row += 4) {
    const int c = min(sCnt[row], cap);
    if (c + sNeed[row] > cap) compact_row(sBuf + row * cap, c, k, lane, &sTau[row], &sCnt[row]);
  }
}

// ---- the row prologue of k_topk, k_retrieve and k_sample (thread tid < TOPK_TU, before the first barrier).  Macros
// for the walk's reason (below): as functions they reorder the prologue's stores.  They name `tid`.

// Row ROW of the N: its user (-1 past N) and where its sorted seen row lies (nothing without a CSR).  Declares `row`,
// `live` (the row is there) and `u` for the kernel's own fields.
#define BPR_STAGE_USER_ROW(ROW, N, USERS, INDPTR, INDICES, SUSER, SSEENLO, SSEENLEN) \
  const int64_t row = (ROW);                                                         \
  const bool live = row < (N);                                                       \
  const int u = live ? (USERS)[row] : -1;                                            \
  {                                                                                  \
    int64_t lo_ = 0;                                                                 \
    int len_ = 0;                                                                    \
    if (live && (INDPTR) != nullptr && (INDICES) != nullptr) {                       \
      lo_ = (INDPTR)[u];                                                             \
      len_ = (int)((INDPTR)[u + 1] - lo_);                                           \
    }                                                                                \
    (SUSER)[tid] = u;                                                                \
    (SSEENLO)[tid] = lo_;                                                            \
    (SSEENLEN)[tid] = len_;                                                          \
  }

// Nothing kept yet: everything beats tau; a row that takes nothing (TAKES false: past n): nothing does.  What follows
// STAU is the kernel's own per-row reset, if it has one (k_retrieve's sChecked), at the place it has always had.
#define BPR_OPEN_SELECTION_ROW(TAKES, SCNT, SNEED, STAU, ...) \
  (SCNT)[tid] = 0;                                            \
  (SNEED)[tid] = 0;                                           \
  __VA_ARGS__;                                                \
  (STAU)[tid] = (TAKES) ? bpr::Cand{-INFINITY, INT_MAX} : bpr::Cand{INFINITY, -1}

// ---- the walk: 256 threads, TOPK_TU rows, the table tiles [FIRST, T1) past them (the contract: the head of this
// file).  A macro pair, for BPR_STASH_CHUNK's reason: as a function that takes the kernel's pieces as lambdas, by
// value or by reference, forced inline or not, every instantiation of k_topk came out rescheduled, with other register
// and spill counts (profiles/serving_walk_resources.md); expanded in place, the loop compiles to the parent's
// instructions.  Being macros they have no scope: they are for the kernels of namespace bpr, they name `tid`, `w`,
// `r`, `h` as every serving kernel declares them, and they declare `t`, `acc0`, `acc1` for the code between them,
// which is the tile's epilogue: register q of the lane is staged table row 32 w + 4 h + (q & 3) + 8 (q >> 2) of
// tile t against rows r (acc0) and 32 + r (acc1).  One walk per scope, BPR_WALK_LANE before it (k_retrieve: once,
// outside its loop over units).  The kernel passes what differs:
//   VEC, SKIP        16-byte or element loads; whether TILE_FROM leaves tiles out
//   FIRST, T1        the tiles; FIRST = TILE_FROM(t0)
//   TABLE, T         which table row is staged as row `row` of tile t: j = TABLE.row(t, row) of T, [.][D], where
//                    TABLE.has(j), else zeros (table_tiles: the rows in their order).  The load itself is written
//                    here: behind a call it is scheduled differently.
//   X, D, SROW       the rows' table, [.][D], and the rows' ids in it, [TOPK_TU] in LDS, -1 for zeros
//   ST, SX           the staged chunks, [TOPK_TI][TOPK_LD] and [TOPK_TU][TOPK_LD]
//   TILE_FROM(t)     the first tile at or after t that is walked, or T1 (without SKIP: t)
//   FETCHED(t, c), STASHED(t, c)   what else travels with chunk c of tile t (walk_nop for nothing; k_neighbors' norms
//                    at c == 0): called when the chunk has been asked for, global -> registers, and when it has been
//                    written to LDS, before the barrier

// the plain table side: tile t is rows TOPK_TI t .. + TOPK_TI - 1 of the N rows of T
struct table_tiles {
  int64_t N;
  __device__ __forceinline__ int64_t row(int64_t t, int row) const { return t * TOPK_TI + row; }
  __device__ __forceinline__ bool has(int64_t j) const { return j < N; }
};

struct walk_nop {
  __device__ __forceinline__ void operator()(int64_t, int) const {}
};

// the lane's constants of a walk: the chunks of a row and where the lane reads its rows of the staged chunks
#define BPR_WALK_LANE(D, ST, SX)                                              \
  const int walk_nch_ = ((D) + bpr::TOPK_KC - 1) / bpr::TOPK_KC;              \
  const float* const walk_ta_ = (ST) + (32 * w + r) * bpr::TOPK_LD + 4 * h;   \
  const float* const walk_xb0_ = (SX) + r * bpr::TOPK_LD + 4 * h;             \
  const float* const walk_xb1_ = (SX) + (32 + r) * bpr::TOPK_LD + 4 * h

#define BPR_WALK_TILES_BEGIN(VEC, SKIP, FIRST, T1, TABLE, T, X, D, SROW, ST, SX, TILE_FROM, FETCHED, STASHED)         \
  /* the next chunk travels global -> registers while the current one is multiplied, then registers -> LDS */         \
  float4 walk_treg_[4], walk_xreg_[2];                                                                                \
  auto walk_fetch_ = [&](int64_t t_, int c_) {                                                                        \
    const int kc_ = c_ * bpr::TOPK_KC;                                                                                \
    _Pragma("unroll") for (int m_ = 0; m_ < 4; ++m_) {                                                                \
      const int f_ = tid + 256 * m_, row_ = f_ >> 3, kk_ = kc_ + 4 * (f_ & 7);                                        \
      const int64_t j_ = (TABLE).row(t_, row_);                                                                       \
      walk_treg_[m_] = (TABLE).has(j_) ? bpr::load4<VEC>((T) + j_ * (D), kk_, (D)) : make_float4(0.f, 0.f, 0.f, 0.f); \
    }                                                                                                                 \
    _Pragma("unroll") for (int m_ = 0; m_ < 2; ++m_) {                                                                \
      const int f_ = tid + 256 * m_, row_ = f_ >> 3, kk_ = kc_ + 4 * (f_ & 7);                                        \
      const int u_ = (SROW)[row_];                                                                                    \
      walk_xreg_[m_] = u_ >= 0 ? bpr::load4<VEC>((X) + (int64_t)u_ * (D), kk_, (D)) : make_float4(0.f, 0.f, 0.f, 0.f); \
    }                                                                                                                 \
    FETCHED(t_, c_);                                                                                                  \
  };                                                                                                                  \
  auto walk_stash_ = [&]() {                                                                                          \
    BPR_STASH_CHUNK((ST), walk_treg_, 4, tid, 256);                                                                   \
    BPR_STASH_CHUNK((SX), walk_xreg_, 2, tid, 256);                                                                   \
  };                                                                                                                  \
  /* SKIP: walk_tn_ is the walked tile after the current one, found once a tile for the prefetch and the step.       \
     Written so that without SKIP the loop is `for (t = FIRST; t < T1; ++t)` to the compiler                         \
     (profiles/item_filter_resources.md). */                                                                          \
  int64_t walk_tn_ = 0;                                                                                               \
  auto walk_next_ = [&](int64_t t_) -> int64_t { return (SKIP) ? walk_tn_ : t_ + 1; };                                \
  const int64_t walk_first_ = (FIRST);                                                                                \
  if (walk_first_ < (T1)) walk_fetch_(walk_first_, 0);                                                                \
  for (int64_t t = walk_first_; t < (T1); t = walk_next_(t)) {                                                        \
    if constexpr (SKIP) walk_tn_ = TILE_FROM(t + 1);                                                                  \
    bpr::f32x16 acc0 = {0.f}, acc1 = {0.f};                                                                           \
    _Pragma("unroll") for (int q_ = 0; q_ < 16; ++q_) acc0[q_] = acc1[q_] = 0.f;                                      \
    for (int c_ = 0; c_ < walk_nch_; ++c_) {                                                                          \
      __syncthreads(); /* every wave is done with the chunk before, and with what the tile before left in LDS */      \
      walk_stash_();                                                                                                  \
      STASHED(t, c_);                                                                                                 \
      __syncthreads(); /* the chunk is whole */                                                                       \
      if (c_ + 1 < walk_nch_) walk_fetch_(t, c_ + 1);                                                                 \
      else if (walk_next_(t) < (T1)) walk_fetch_(walk_next_(t), 0);                                                   \
      bpr::mfma_chunk2(walk_ta_, walk_xb0_, walk_xb1_, acc0, acc1);                                                   \
    }
#define BPR_WALK_TILES_END }

}  // namespace bpr
