// bpr_foldin_scored_plan.h — how a fold-in launch with SCORED negatives (k_foldin_scored, bpr_foldin_scored.hip:
// dynamic negatives or the WARP objective, bpr_scored.h) is laid out: the group shape and grid of bpr_foldin_plan.h,
// the seen structure of bpr_foldin_adaptive_plan.h (the same rule, the same words), the argument ranges of
// bpr_scored_plan.h, and how many workgroups of each instantiation a CU holds.  Integer arithmetic on the shape only:
// no HIP, no context (plain C++17; tests/test_foldin_scored_cpu.py pins it through `bpr_test_foldin_scored_plan`, and
// tests/foldin_scored_plan_check.cpp under the host sanitizers).
//
// Seen structure.  A scored draw asks "seen?" once per lane and round of candidates (a round or two per triple for
// all but nearly complete rows), and a row is drawn for epochs * m times, so each group keeps an I-bit bitmap of its
// row in LDS (built once per row) when the workgroup's bitmaps fit FOLDIN_ADAPTIVE_LDS_MAX; beyond that a draw
// searches the row's CSR slice.  The exact pick by rank (no candidate accepted) reads the slice in either case.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bpr_foldin_adaptive_plan.h"
#include "bpr_scored_plan.h"

namespace bpr {

// Triples whose positive (id, and for BPR_NEG_DYNAMIC its row and bias) is fetched ahead of the draw -> update chain
// (E <= 4; halved per doubling of E past 4: the ring lives in VGPRs).  2 is k_foldin's measured depth
// (bpr_foldin_plan.h); no other depth of THIS kernel has been measured.  What the ring can hide is small here: the
// draw's own chunk of candidate rows is a dependent round trip per triple that nothing can run ahead of.
#ifndef BPR_FOLDIN_SCORED_PF
#define BPR_FOLDIN_SCORED_PF 2
#endif
constexpr int FOLDIN_SCORED_PF = BPR_FOLDIN_SCORED_PF;
constexpr int foldin_scored_pf(int E) { return foldin_pf_at(FOLDIN_SCORED_PF, E); }

// Workgroups of 4 waves a CU holds of an instantiation: FOLDIN_RESIDENT (4 waves per SIMD, 128 VGPRs each) where its
// VGPRs allow.  Four bitmap instantiations take 131 - 133 (DESIGN 4.7.2 has the table: the chunk of candidate rows in
// flight beside the ring, or beside 16 registers a row at E = 16) and are capped at 3; none uses scratch.  The rule
// is written from the compiler's remarks, not derived from them: profiles/foldin_scored_resources.md says how to
// take the table again after a toolchain or kernel change (a stale rule costs time, never correctness).
constexpr int foldin_scored_resident(int E, int kind, bool bitmap) {
  return bitmap && (E == 16 || (E == 4 && kind == BPR_NEG_DYNAMIC)) ? FOLDIN_RESIDENT - 1 : FOLDIN_RESIDENT;
}

struct FoldinScoredPlan {
  int G, E, block, groups_per_block, pf;  // as FoldinPlan
  int bitmap;                             // 1: per-group LDS bitmap, 0: the row's CSR slice
  int bm_words;                           // 32-bit words of one group's bitmap (a multiple of 4), 0 without
  int64_t lds_bytes;                      // dynamic LDS of a workgroup
  int resident;                           // workgroups per CU the grid is capped at
  int64_t groups, grid;
};

// n >= 0, I >= 1, 1 <= d <= FOLDIN_MAX_D, kind a scored one (checked by the callers).  A forced bitmap that does not
// fit is not taken.
inline FoldinScoredPlan plan_foldin_scored(int64_t n, int64_t I, int d, int kind, int cus = FOLDIN_CUS,
                                           int seen_mode = FOLDIN_SEEN_AUTO) {
  FoldinScoredPlan p = {};
  foldin_ge(d, &p.G, &p.E);
  p.block = FOLDIN_BLOCK;
  p.groups_per_block = FOLDIN_BLOCK / p.G;
  p.pf = foldin_scored_pf(p.E);
  const int64_t words = foldin_bitmap_words(I);
  const int64_t bytes = words * 4 * p.groups_per_block;
  p.bitmap = (seen_mode != FOLDIN_SEEN_CSR && bytes <= FOLDIN_ADAPTIVE_LDS_MAX) ? 1 : 0;
  p.bm_words = p.bitmap ? (int)words : 0;
  p.lds_bytes = p.bitmap ? bytes : 0;
  const int by_regs = foldin_scored_resident(p.E, kind, p.bitmap != 0);
  p.resident = p.bitmap ? (int)std::min<int64_t>(by_regs, FOLDIN_ADAPTIVE_LDS_CU / p.lds_bytes) : by_regs;
  foldin_groups_grid(n, cus, p.resident, p.groups_per_block, &p.groups, &p.grid);
  return p;
}

}  // namespace bpr
