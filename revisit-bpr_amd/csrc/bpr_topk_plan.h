// bpr_topk_plan.h — how a fused top-K launch (k_topk, bpr_topk.hip) is laid out: tile sizes, item slices, the
// per-row candidate buffer, dynamic LDS and the device workspace.  Integer arithmetic on the shape only: no HIP
// (plain C++17; tests/test_recommend_cpu.py pins it on the CPU through `bpr_test_topk_plan`).
//
// A workgroup of 256 threads owns TOPK_TU users and walks the item tiles of its slice, TOPK_TI items at a time,
// TOPK_KC features at a time.  Both operands are streamed through LDS in [rows][TOPK_KC] chunks, so the LDS a
// workgroup needs does not depend on d; what it does depend on is k: every row keeps a buffer of k + TOPK_TI
// (score, id) candidates — the k best of the last compaction plus whatever one item tile can append at worst.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace bpr {

constexpr int TOPK_MAX = 128;         // largest k (the reference configs' largest cutoff is 100)
constexpr int TOPK_TU = 64;           // users of a workgroup
constexpr int TOPK_TI = 128;          // items of a tile (4 waves x 32)
constexpr int TOPK_KC = 32;           // features of a staged chunk
constexpr int TOPK_LD = TOPK_KC + 4;  // floats of a staged row: 16-byte LDS reads of 32 rows fall on distinct banks
constexpr int TOPK_MAX_SLICES = 64;   // the merge kernel holds slices x k candidates of a row in LDS (<= 64 KiB)
constexpr int TOPK_CUS = 256;         // CUs a launch is sized for (MI355X)

struct TopkPlan {
  int64_t user_tiles, item_tiles;
  int slices;        // item slices (grid.y); 1 = the kernel writes the result itself, no merge
  int cap;           // candidates a row's buffer holds
  size_t lds;        // dynamic LDS of k_topk
  size_t merge_lds;  // dynamic LDS of k_topk_merge (0 without a merge)
  int64_t ws_bytes;  // device workspace: the slices' partial results, [n, slices, k] scores then ids
};

// staged operands, then per row: candidates, threshold (score, id), count, pending count, user id, seen row (start, length)
inline size_t topk_lds_bytes(int k) {
  const size_t stage = sizeof(float) * (size_t)(TOPK_TU + TOPK_TI) * TOPK_LD;
  const size_t rows = (size_t)TOPK_TU * ((size_t)(k + TOPK_TI) * 8 + 8 + 4 + 4 + 4 + 8 + 4);
  return stage + rows;
}

// slices when the caller leaves the choice (item_slices == 0): one per CU the user tiles leave idle
inline int topk_auto_slices(int64_t user_tiles, int64_t item_tiles, int cus) {
  if (user_tiles >= cus) return 1;
  const int64_t want = (cus + user_tiles - 1) / user_tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, std::min<int64_t>(item_tiles, TOPK_MAX_SLICES)));
}

inline int64_t topk_partial_bytes(int64_t n, int slices, int k) {
  return slices <= 1 ? 0 : n * (int64_t)slices * k * 8;
}

// n >= 0, I >= 1, 1 <= k <= TOPK_MAX, 0 <= item_slices <= TOPK_MAX_SLICES (checked by the callers)
inline TopkPlan plan_topk(int64_t n, int64_t I, int k, int item_slices, int cus = TOPK_CUS) {
  TopkPlan p = {};
  p.user_tiles = (n + TOPK_TU - 1) / TOPK_TU;
  p.item_tiles = (I + TOPK_TI - 1) / TOPK_TI;
  p.slices = item_slices > 0 ? (int)std::min<int64_t>(item_slices, p.item_tiles)
                             : topk_auto_slices(std::max<int64_t>(p.user_tiles, 1), p.item_tiles, cus);
  p.cap = k + TOPK_TI;
  p.lds = topk_lds_bytes(k);
  p.merge_lds = p.slices > 1 ? (size_t)p.slices * k * 8 + sizeof(int) * (TOPK_MAX_SLICES + 1) : 0;
  p.ws_bytes = topk_partial_bytes(n, p.slices, k);
  return p;
}

// first item tile of slice s (s == slices: one past the last): the slices cover the tiles exactly once
inline int64_t topk_slice_tile(const TopkPlan& p, int s) { return p.item_tiles * s / p.slices; }

// What bpr_topk_workspace answers.  A given slice count: the partial results.  The library's choice: the largest
// need of any n' <= n, so that the answer never shrinks as n grows (the choice drops to one slice, and no
// workspace, once the user tiles fill the chip: at most TOPK_CUS - 1 tiles ever ask for one).
inline int64_t topk_workspace_bytes(int64_t n, int64_t I, int k, int item_slices, int cus = TOPK_CUS) {
  if (item_slices > 0) return plan_topk(n, I, k, item_slices, cus).ws_bytes;
  int64_t best = 0;
  const int64_t tiles = (n + TOPK_TU - 1) / TOPK_TU;
  for (int64_t t = 1; t <= std::min<int64_t>(tiles, cus - 1); ++t)
    best = std::max(best, plan_topk(std::min<int64_t>(n, t * TOPK_TU), I, k, 0, cus).ws_bytes);
  return best;
}

}  // namespace bpr
