// bpr_sample_plan.h — how a sampling launch (k_sample, bpr_sample.hip) is laid out.  It is k_topk's plan
// (bpr_topk_plan.h: tiles, slices, the candidate buffer of 8-byte (key, id) pairs, dynamic LDS) plus the workspace
// of the optional log_z: 8 bytes — a running maximum and a rescaled sum — per row and slice, with one slice too
// (bpr_sample_finish turns them into log_z).  Integer arithmetic on the shape only: no HIP (plain C++17;
// tests/sample_plan_check.cpp pins it on the CPU under the host sanitizers).
//
// LDS.  The candidate stays at 8 bytes, so the budget is k_topk's: 160,768 B at k = 128, one workgroup per CU.  What
// log_z needs per item tile — a 128-bit seen mask per row and the four waves' partial (max, sum) per row — lives in
// the operand staging area, which is idle between a tile's last MFMA and the next tile's first chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bpr_topk_plan.h"

namespace bpr {

constexpr size_t SAMPLE_LDS_CU = 160 * 1024;  // LDS of a gfx950 CU
// per item tile, in the staging area: seen masks [TU][TI / 32] u32, then partials [4 waves][TU] (max, sum)
constexpr size_t SAMPLE_SCRATCH_BYTES = (size_t)TOPK_TU * (TOPK_TI / 32) * 4 + (size_t)4 * TOPK_TU * 8;
constexpr size_t SAMPLE_STAGE_Q_BYTES = sizeof(float) * (size_t)TOPK_TI * TOPK_LD;  // what the scratch aliases
static_assert(SAMPLE_SCRATCH_BYTES <= SAMPLE_STAGE_Q_BYTES, "the log_z scratch must fit into the item staging area");

struct SamplePlan {
  TopkPlan topk;     // tiles, slices, cap, lds, merge_lds; ws_bytes = the slices' partial results
  int64_t lz_bytes;  // the slices' (max, sum) pairs, [n, slices] x 8 bytes; 0 when log_z is not wanted
  int64_t ws_bytes;  // topk.ws_bytes (first), then lz_bytes
};

inline size_t sample_lds_bytes(int k) { return topk_lds_bytes(k); }

// n >= 0, I >= 1, 1 <= k <= TOPK_MAX, 0 <= item_slices <= TOPK_MAX_SLICES (checked by the callers)
inline SamplePlan plan_sample(int64_t n, int64_t I, int k, int item_slices, bool want_log_z, int cus = TOPK_CUS) {
  SamplePlan p = {};
  p.topk = plan_topk(n, I, k, item_slices, cus);
  p.lz_bytes = want_log_z ? n * (int64_t)p.topk.slices * 8 : 0;
  p.ws_bytes = p.topk.ws_bytes + p.lz_bytes;
  return p;
}

// What bpr_sample_workspace answers: as topk_workspace_bytes — a given slice count: that call's need; the library's
// choice: the largest need of any n' <= n, so that the answer never shrinks as n grows.
inline int64_t sample_workspace_bytes(int64_t n, int64_t I, int k, int item_slices, bool want_log_z,
                                      int cus = TOPK_CUS) {
  if (item_slices > 0) return plan_sample(n, I, k, item_slices, want_log_z, cus).ws_bytes;
  // past cus - 1 user tiles the choice is one slice: no partial results, and 8 bytes per row for log_z
  int64_t best = plan_sample(n, I, k, 0, want_log_z, cus).ws_bytes;
  const int64_t tiles = (n + TOPK_TU - 1) / TOPK_TU;
  for (int64_t t = 1; t <= std::min<int64_t>(tiles, cus - 1); ++t)
    best = std::max(best, plan_sample(std::min<int64_t>(n, t * TOPK_TU), I, k, 0, want_log_z, cus).ws_bytes);
  return best;
}

}  // namespace bpr
