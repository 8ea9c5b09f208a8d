// bpr_retrieve_plan.h — how a deep top-K launch (k_retrieve, bpr_retrieve.hip) is laid out: the per-row candidate
// buffer, the sort scratch, dynamic LDS, item slices, the persistent grid and the device workspace.  Integer
// arithmetic on the shape only: no HIP (plain C++17; tests/test_retrieve_cpu.py pins it on the CPU through
// `bpr_test_retrieve_plan`, tests/retrieve_plan_check.cpp sweeps it alone under the host sanitizers).
//
// Tiles are k_topk's (bpr_topk_plan.h): a workgroup of 256 threads owns TOPK_TU users and walks the item tiles of
// its slice, TOPK_TI items and TOPK_KC features at a time.  What k_topk keeps in LDS — k + TOPK_TI candidates for
// each of its 64 rows — is what stops it at k = 128.  Here the rows' buffers are device memory: a workgroup owns one
// block of TOPK_TU x cap candidates in the workspace, and LDS holds only the staged operands, the rows' meta data and
// the scratch in which 4 rows at a time (one per wave) are sorted.  A bounded number of persistent workgroups walks
// the (user tile, slice) pairs, so the blocks do not grow with n.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bpr_topk_plan.h"

namespace bpr {

constexpr int RETRIEVE_MAX = 1024;             // largest k
constexpr int RETRIEVE_SLICE_K = 8192;         // slices x k at most: what k_topk_merge holds of a row (64 x 128 today)
constexpr size_t RETRIEVE_LDS_CU = 160 * 1024;  // LDS of a CU (gfx950)

struct RetrievePlan {
  int64_t user_tiles, item_tiles;
  int slices;          // item slices; 1 = the kernel writes the result itself, no merge
  int cap;             // candidates a row's buffer holds: a power of two, >= max(k + TOPK_TI, 2 k)
  size_t lds;          // dynamic LDS of k_retrieve
  size_t merge_lds;    // dynamic LDS of k_topk_merge (0 without a merge)
  int64_t units;       // (user tile, slice) pairs: unit x is slice x % slices of user tile x / slices
  int64_t grid;        // persistent workgroups: workgroup b walks the units b, b + grid, ...
  int64_t part_bytes;  // workspace, first part: the slices' partial results, [n, slices, k] scores then ids
  int64_t buf_bytes;   // workspace, second part: [grid][TOPK_TU][cap] (score, id) candidates
  int64_t ws_bytes;    // part_bytes + buf_bytes
};

// The buffer of a row.  It must take the k best of the last compaction plus whatever one item tile appends at worst
// (k + TOPK_TI); twice k makes every compaction free at least k slots, so that a row is sorted once per k appends
// and not once per tile; and a power of two lets the bitonic network sort a full buffer in a scratch of its size.
inline int retrieve_cap(int k) {
  const int want = std::max(k + TOPK_TI, 2 * k);
  int cap = 1;
  while (cap < want) cap <<= 1;
  return cap;
}

// staged operands; the sort scratch of 4 rows; then per row: threshold (score, id), seen row start, count, pending
// count, user id, seen row length, and how many of the row's candidates are known to be unseen
inline size_t retrieve_lds_bytes(int k) {
  const size_t stage = sizeof(float) * (size_t)(TOPK_TU + TOPK_TI) * TOPK_LD;
  const size_t scratch = (size_t)4 * retrieve_cap(k) * 8;
  const size_t rows = (size_t)TOPK_TU * (8 + 8 + 4 + 4 + 4 + 4 + 4);
  return stage + scratch + rows;
}

// the most slices a row's merge takes at this k
inline int retrieve_max_slices(int k) { return std::max(1, std::min(TOPK_MAX_SLICES, RETRIEVE_SLICE_K / k)); }

// workgroups a launch keeps resident at most: as many per CU as the LDS lets in, two at most
inline int64_t retrieve_grid_max(int k, int cus) {
  return (int64_t)cus * (2 * retrieve_lds_bytes(k) <= RETRIEVE_LDS_CU ? 2 : 1);
}

// n >= 0, I >= 1, 1 <= k <= RETRIEVE_MAX, 0 <= item_slices <= TOPK_MAX_SLICES (checked by the callers); a given
// slice count above what the merge or the item tiles take is reduced, not refused
inline RetrievePlan plan_retrieve(int64_t n, int64_t I, int k, int item_slices, int cus = TOPK_CUS) {
  RetrievePlan p = {};
  p.user_tiles = (n + TOPK_TU - 1) / TOPK_TU;
  p.item_tiles = (I + TOPK_TI - 1) / TOPK_TI;
  const int64_t most = std::min<int64_t>(retrieve_max_slices(k), p.item_tiles);
  p.slices = (int)std::min<int64_t>(
      most, item_slices > 0 ? item_slices : topk_auto_slices(std::max<int64_t>(p.user_tiles, 1), p.item_tiles, cus));
  p.cap = retrieve_cap(k);
  p.lds = retrieve_lds_bytes(k);
  p.merge_lds = p.slices > 1 ? (size_t)p.slices * k * 8 + sizeof(int) * (TOPK_MAX_SLICES + 1) : 0;
  p.units = p.user_tiles * p.slices;
  p.grid = std::min<int64_t>(p.units, retrieve_grid_max(k, cus));
  p.part_bytes = topk_partial_bytes(n, p.slices, k);
  p.buf_bytes = p.grid * TOPK_TU * p.cap * 8;
  p.ws_bytes = p.part_bytes + p.buf_bytes;
  return p;
}

// first item tile of slice s (s == slices: one past the last): the slices cover the tiles exactly once
inline int64_t retrieve_slice_tile(const RetrievePlan& p, int s) { return p.item_tiles * s / p.slices; }

// What bpr_retrieve_workspace answers.  A given slice count: the call's own need.  The library's choice: the
// largest need of any n' <= n, so that the answer never shrinks as n grows (as topk_workspace_bytes: the choice drops
// to one slice, and no partial results, once the user tiles fill the chip).  Past the persistent grid's reach only
// the partial results of a given slice count grow with n.
inline int64_t retrieve_workspace_bytes(int64_t n, int64_t I, int k, int item_slices, int cus = TOPK_CUS) {
  int64_t best = plan_retrieve(n, I, k, item_slices, cus).ws_bytes;
  if (item_slices > 0) return best;
  const int64_t tiles = (n + TOPK_TU - 1) / TOPK_TU;
  for (int64_t t = 1; t <= std::min<int64_t>(tiles, cus - 1); ++t)
    best = std::max(best, plan_retrieve(std::min<int64_t>(n, t * TOPK_TU), I, k, 0, cus).ws_bytes);
  return best;
}

}  // namespace bpr
