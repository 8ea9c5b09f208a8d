// bpr_topk_shared.h — what the serving kernels have in common (k_topk, bpr_topk.hip; k_rank, bpr_rank.hip;
// k_neighbors, bpr_neighbors.hip; k_rerank, bpr_rerank.hip; k_diversify, bpr_diversify.hip), each piece defined once.
// Device side: the guarded load of 4 features (load4), the registers -> LDS copy of a staged chunk (stash_piece,
// BPR_STASH_CHUNK), the dot product's chain as MFMAs and as fmaf (mfma_chunk2, mfma_block1, fma_chain8), the result order (Cand,
// better), rank-by-counting compaction of a candidate buffer (compact_row) and the selection step k_topk and
// k_neighbors run alike (compact_overflowing_rows).  Device code only: what the entry points' host sides share is
// bpr_serving_host.h.  What differs between the kernels — where a staged row comes from, eligibility, what a score
// becomes — stays in their files.
//
// Every piece here compiles to the instructions of the same statements written out in each kernel; the pieces that
// did not in any form tried are still in the kernels' files (profiles/topk_shared_resources.md names them).  No division and no square root: the header means the same under the
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

}  // namespace bpr
