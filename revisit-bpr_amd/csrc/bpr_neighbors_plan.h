// bpr_neighbors_plan.h — how a fused neighbour top-K launch (k_neighbors, bpr_neighbors.hip) is laid out: dynamic
// LDS, slices of the table and the device workspace.  Integer arithmetic on the shape only: no HIP (plain C++17;
// tests/test_neighbors_cpu.py pins it on the CPU through `bpr_test_neighbors_plan`).
//
// The tiling is k_topk's (bpr_topk_plan.h): a workgroup of 256 threads owns TOPK_TU queries and walks the table
// tiles of its slice, TOPK_TI rows at a time, TOPK_KC features at a time, both operands staged through LDS in
// [rows][TOPK_LD] chunks; every query keeps a buffer of k + TOPK_TI (score, id) candidates.  Slices are chosen as
// for k_topk — the same counts for the same (n, N, k) — so the two kernels can be timed side by side.  What differs
// is the per-query state (the excluded id and the query's reciprocal norm instead of a seen row) and, under the
// cosine metric, one reciprocal norm per row of the staged table tile and per table row / query in the workspace.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bpr_topk_plan.h"

namespace bpr {

constexpr int NBR_DOT = 0, NBR_COSINE = 1;  // BPR_SIM_DOT, BPR_SIM_COSINE (bprcore.h)
constexpr size_t NBR_LDS_LIMIT = 163840;    // LDS of a CU (gfx950): one workgroup at k = TOPK_MAX must fit

struct NeighborsPlan {
  TopkPlan t;             // tiles, slices, candidate buffer, merge LDS, partial results: k_topk's
  size_t lds;             // dynamic LDS of k_neighbors
  int64_t partial_bytes;  // [n, slices, k] scores then ids (0 with one slice)
  int64_t norm_bytes;     // cosine: rn of the N table rows, then of the n queries, fp32
  int64_t ws_bytes;       // partial_bytes + norm_bytes
};

// staged operands, the table tile's reciprocal norms, then per query: candidates, threshold (score, id), count,
// pending count, row of X, excluded id, reciprocal norm
inline size_t neighbors_lds_bytes(int k) {
  const size_t stage = sizeof(float) * (size_t)(TOPK_TU + TOPK_TI) * TOPK_LD + sizeof(float) * TOPK_TI;
  const size_t rows = (size_t)TOPK_TU * ((size_t)(k + TOPK_TI) * 8 + 8 + 4 + 4 + 4 + 4 + 4);
  return stage + rows;
}
static_assert((size_t)(TOPK_TU + TOPK_TI) * TOPK_LD * 4 + TOPK_TI * 4 +
                      (size_t)TOPK_TU * ((size_t)(TOPK_MAX + TOPK_TI) * 8 + 28) <= NBR_LDS_LIMIT,
              "one workgroup of k_neighbors at the largest k must fit a CU's LDS");

inline int64_t neighbors_norm_bytes(int64_t n, int64_t N, int metric) {
  return metric == NBR_COSINE ? (N + n) * 4 : 0;
}

// n >= 0, N >= 1, 1 <= k <= TOPK_MAX, 0 <= item_slices <= TOPK_MAX_SLICES, metric known (checked by the callers)
inline NeighborsPlan plan_neighbors(int64_t n, int64_t N, int k, int metric, int item_slices, int cus = TOPK_CUS) {
  NeighborsPlan p = {};
  p.t = plan_topk(n, N, k, item_slices, cus);
  p.lds = neighbors_lds_bytes(k);
  p.partial_bytes = p.t.ws_bytes;
  p.norm_bytes = neighbors_norm_bytes(n, N, metric);
  p.ws_bytes = p.partial_bytes + p.norm_bytes;
  return p;
}

// What bpr_neighbors_workspace answers: the partial results as bpr_topk_workspace counts them (a given slice count:
// that call's; the library's choice: the largest need of any n' <= n, so the answer never shrinks as n grows) plus
// the norms, which grow with n.
inline int64_t neighbors_workspace_bytes(int64_t n, int64_t N, int k, int metric, int item_slices,
                                         int cus = TOPK_CUS) {
  return topk_workspace_bytes(n, N, k, item_slices, cus) + neighbors_norm_bytes(n, N, metric);
}

}  // namespace bpr
