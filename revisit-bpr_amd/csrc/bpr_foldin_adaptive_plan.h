// bpr_foldin_adaptive_plan.h — how a fold-in launch with adaptive negatives (k_foldin_adaptive,
// bpr_foldin_adaptive.hip) is laid out: the group shape and grid of bpr_foldin_plan.h, plus the structure that
// answers "has this user seen item c?" and the LDS it takes.  Integer arithmetic on the shape only: no HIP, no
// context (plain C++17; tests/test_foldin_adaptive_cpu.py pins it through `bpr_test_foldin_adaptive_plan`).
//
// Seen structure.  The adaptive walk asks 4 questions per lane and trip, and a row is walked epochs * m times, so
// each group keeps an I-bit bitmap of its row in LDS (built once per row) when the workgroup's bitmaps fit
// FOLDIN_ADAPTIVE_LDS_MAX; beyond that the walk searches the row's CSR slice.  Both are predicates of the same
// set: the negatives do not depend on the choice.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bpr_foldin_plan.h"

namespace bpr {

constexpr int64_t FOLDIN_ADAPTIVE_LDS_MAX = 64 * 1024;  // bytes of bitmaps per workgroup (the launch's default limit)
constexpr int64_t FOLDIN_ADAPTIVE_LDS_CU = 160 * 1024;  // LDS of a CU (CDNA4)
// Triples whose positive row and randoms are fetched ahead of the draw -> negative row -> update chain (E <= 4;
// halved per doubling of E past 4: the ring lives in VGPRs).  Measured on an MI355X, 10,000 users, 5 epochs, bitmap
// (profiles/foldin_probe_adaptive.txt): ML-20M shape, d = 128: 100.2 / 96.3 / 94.2 ms at depth 1 / 2 / 4; MSD shape,
// d = 256: 16.66 / 16.19 / 15.78 ms — one process per depth; against the uniform kernel in the same process 1.09 /
// 1.03 / 1.02 and 1.03 / 0.99 / 0.98.  Depth 4 is clearly ahead of depth 2 on the MSD shape only; on the ML-20M shape
// the two are within noise.  Depth 4 still leaves the 4 waves per SIMD the grid cap asks for.
#ifndef BPR_FOLDIN_ADAPTIVE_PF
#define BPR_FOLDIN_ADAPTIVE_PF 4
#endif
constexpr int FOLDIN_ADAPTIVE_PF = BPR_FOLDIN_ADAPTIVE_PF;
constexpr int foldin_adaptive_pf(int E) { return foldin_pf_at(FOLDIN_ADAPTIVE_PF, E); }

enum { FOLDIN_SEEN_AUTO = 0, FOLDIN_SEEN_CSR = 1, FOLDIN_SEEN_BITMAP = 2 };  // seen_mode (tests force 1 or 2)

struct FoldinAdaptivePlan {
  int G, E, block, groups_per_block, pf;  // as FoldinPlan
  int bitmap;                             // 1: per-group LDS bitmap, 0: the row's CSR slice
  int bm_words;                           // 32-bit words of one group's bitmap (a multiple of 4), 0 without
  int64_t lds_bytes;                      // dynamic LDS of a workgroup
  int resident;                           // workgroups per CU the grid is capped at
  int64_t groups, grid;
};

// words of an I-bit bitmap, rounded up to whole 16-byte vectors
inline int64_t foldin_bitmap_words(int64_t I) { return ((I + 31) / 32 + 3) / 4 * 4; }

// n >= 0, I >= 1, 1 <= d <= FOLDIN_MAX_D (checked by the callers).  A forced bitmap that does not fit is not taken.
inline FoldinAdaptivePlan plan_foldin_adaptive(int64_t n, int64_t I, int d, int cus = FOLDIN_CUS,
                                               int seen_mode = FOLDIN_SEEN_AUTO) {
  FoldinAdaptivePlan p = {};
  foldin_ge(d, &p.G, &p.E);
  p.block = FOLDIN_BLOCK;
  p.groups_per_block = FOLDIN_BLOCK / p.G;
  p.pf = foldin_adaptive_pf(p.E);
  const int64_t words = foldin_bitmap_words(I);
  const int64_t bytes = words * 4 * p.groups_per_block;
  p.bitmap = (seen_mode != FOLDIN_SEEN_CSR && bytes <= FOLDIN_ADAPTIVE_LDS_MAX) ? 1 : 0;
  p.bm_words = p.bitmap ? (int)words : 0;
  p.lds_bytes = p.bitmap ? bytes : 0;
  p.resident = p.bitmap ? (int)std::min<int64_t>(FOLDIN_RESIDENT, FOLDIN_ADAPTIVE_LDS_CU / p.lds_bytes)
                        : FOLDIN_RESIDENT;
  foldin_groups_grid(n, cus, p.resident, p.groups_per_block, &p.groups, &p.grid);
  return p;
}

}  // namespace bpr
