// bpr_rank_plan.h — how a fused ranking launch (k_rank, bpr_rank.hip) is laid out: tile sizes, item slices, the
// per-row target list, dynamic LDS and the device workspace.  Integer arithmetic on the shape only: no HIP (plain
// C++17; tests/test_rank_cpu.py pins it on the CPU through `bpr_test_rank_plan`).
//
// A workgroup of 256 threads owns RANK_TR rows (a row = one user with a list of targets) and walks the item tiles of
// its slice, RANK_TI items at a time, RANK_KC features at a time, exactly as k_topk does (bpr_topk_plan.h): both
// operands are streamed through LDS in [rows][RANK_KC] chunks, so the LDS does not depend on d.  What it holds per
// row is the row's targets: RANK_TMAX (score, id) entries sorted by the result order, a bin per entry plus one, a
// "tied after" counter per entry and the entry's place in the caller's list.
//
// LDS budget (bytes), one workgroup per CU of 160 KiB = 163,840:
//   staged operands    (RANK_TI + RANK_TR) * RANK_LD * 4                  27,648
//   per-row scalars    seen row start 8, target start 8 (+ 16), user 4, seen length 4, targets 4     1,808
//   eligibility mask   RANK_TR * 16                                         1,024
//   sorted targets     RANK_TR * RANK_TMAX * 8                             57,344
//   bins + tied after  RANK_TR * RANK_HT * 4   (RANK_HT = 2 RANK_TMAX + 2) 57,856
//   place in the list  RANK_TR * RANK_TMAX * 2                             14,336
//                                                                         160,016
// RANK_TMAX = 112 is the largest multiple of 16 that fits (128: 178,448).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace bpr {

constexpr int RANK_TMAX = 112;            // targets of a row (longer rows: the caller splits them)
constexpr int RANK_TR = 64;               // rows of a workgroup
constexpr int RANK_TI = 128;              // items of a tile (4 waves x 32)
constexpr int RANK_KC = 32;               // features of a staged chunk
constexpr int RANK_LD = RANK_KC + 4;      // floats of a staged row (as TOPK_LD)
constexpr int RANK_HT = 2 * RANK_TMAX + 2;  // ints of a row's counters: bins [0, TMAX], one pad, tied after [TMAX + 2, ..)
constexpr int RANK_MAX_SLICES = 64;
constexpr int RANK_CUS = 256;             // CUs a launch is sized for (MI355X)

struct RankPlan {
  int64_t row_tiles, item_tiles;
  int slices;        // item slices (grid.y); 1 = the kernel writes the result itself, no workspace, no finish
  size_t lds;        // dynamic LDS of the ranking pass
  size_t pre_lds;    // dynamic LDS of the target-score pass
  int64_t ws_bytes;  // device workspace: [3][n][RANK_TMAX] int32 (bins, tied after, place in the list)
};

inline size_t rank_scalar_bytes() { return (size_t)RANK_TR * 8 + (size_t)(RANK_TR + 2) * 8 + (size_t)RANK_TR * 12; }

inline size_t rank_stage_bytes() { return sizeof(float) * (size_t)(RANK_TR + RANK_TI) * RANK_LD; }

inline size_t rank_lds_bytes() {
  return rank_stage_bytes() + rank_scalar_bytes() + (size_t)RANK_TR * 16 + (size_t)RANK_TR * RANK_TMAX * 8 +
         (size_t)RANK_TR * RANK_HT * 4 + (size_t)RANK_TR * RANK_TMAX * 2;
}

// the target-score pass: staging, the scalars and the owning row of each of a tile's targets
inline size_t rank_pre_lds_bytes() { return rank_stage_bytes() + rank_scalar_bytes() + (size_t)RANK_TI * 4; }

// slices when the caller leaves the choice (item_slices == 0): one per CU the row tiles leave idle
inline int rank_auto_slices(int64_t row_tiles, int64_t item_tiles, int cus) {
  if (row_tiles >= cus) return 1;
  const int64_t want = (cus + row_tiles - 1) / row_tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(item_tiles, RANK_MAX_SLICES)));
}

inline int64_t rank_partial_bytes(int64_t n, int slices) { return slices <= 1 ? 0 : n * (int64_t)RANK_TMAX * 12; }

// n >= 0, I >= 1, 0 <= item_slices <= RANK_MAX_SLICES (checked by the callers)
inline RankPlan plan_rank(int64_t n, int64_t I, int item_slices, int cus = RANK_CUS) {
  RankPlan p = {};
  p.row_tiles = (n + RANK_TR - 1) / RANK_TR;
  p.item_tiles = (I + RANK_TI - 1) / RANK_TI;
  p.slices = item_slices > 0 ? (int)std::min<int64_t>(item_slices, p.item_tiles)
                             : rank_auto_slices(std::max<int64_t>(p.row_tiles, 1), p.item_tiles, cus);
  p.lds = rank_lds_bytes();
  p.pre_lds = rank_pre_lds_bytes();
  p.ws_bytes = rank_partial_bytes(n, p.slices);
  return p;
}

// first item tile of slice s (s == slices: one past the last): the slices cover the tiles exactly once
inline int64_t rank_slice_tile(const RankPlan& p, int s) { return p.item_tiles * s / p.slices; }

// What bpr_rank_workspace answers.  A given slice count: that call's need.  The library's choice: the largest need
// of any n' <= n, so that the answer never shrinks as n grows (the choice drops to one slice, and no workspace, once
// the row tiles fill the chip).
inline int64_t rank_workspace_bytes(int64_t n, int64_t I, int item_slices, int cus = RANK_CUS) {
  if (item_slices > 0) return plan_rank(n, I, item_slices, cus).ws_bytes;
  int64_t best = 0;
  const int64_t tiles = (n + RANK_TR - 1) / RANK_TR;
  for (int64_t t = 1; t <= std::min<int64_t>(tiles, cus - 1); ++t)
    best = std::max(best, plan_rank(std::min<int64_t>(n, t * RANK_TR), I, 0, cus).ws_bytes);
  return best;
}

}  // namespace bpr
