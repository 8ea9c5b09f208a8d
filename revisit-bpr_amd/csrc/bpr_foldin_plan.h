// bpr_foldin_plan.h — how a fold-in launch (k_foldin, bpr_foldin.hip; k_foldin_items, bpr_foldin_items.hip) is laid
// out: group width, elements per lane, block, groups and grid, and what bpr_foldin_adaptive_plan.h builds on.
// Integer arithmetic on the shape only: no HIP, no context (plain C++17; tests/test_foldin_cpu.py pins it on the
// CPU through `bpr_test_foldin_plan`).
//
// One group of G lanes owns one new user at a time and takes rows by ticket, so a launch never needs more groups
// than rows, and never more than the chip holds at once: a group beyond that would only queue behind a resident
// one for a ticket the resident one takes anyway.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bpr_group_shape.h"

namespace bpr {

constexpr int FOLDIN_BLOCK = 256;    // threads of a workgroup: 8 groups of 32 lanes, or 4 of 64
constexpr int FOLDIN_CUS = 256;      // CUs a launch is sized for (MI355X)
constexpr int FOLDIN_RESIDENT = 4;   // workgroups per CU the grid is capped at (16 waves: the kernel's VGPR budget)
constexpr int FOLDIN_MAX_D = 1024;
// Triples whose item rows are in flight ahead of the update chain (E <= 4).  Measured on an MI355X, 10,000 users,
// 5 epochs, sampled negatives (profiles/foldin_probe_pf_sweep.txt): ML-20M shape, d = 128: 102.6 / 99.6 / 107.9 /
// 108.9 ms at depth 1 / 2 / 4 / 8; MSD shape, d = 256: 16.9 / 16.7 / 18.2 / 18.2 ms.
#ifndef BPR_FOLDIN_PF
#define BPR_FOLDIN_PF 2
#endif
constexpr int FOLDIN_PF = BPR_FOLDIN_PF;
// The same for each stage of k_foldin_items.  The default is k_foldin's measured choice; no other depth of THAT
// kernel has been measured.
#ifndef BPR_FOLDIN_ITEMS_PF
#define BPR_FOLDIN_ITEMS_PF BPR_FOLDIN_PF
#endif

struct FoldinPlan {
  int G, E;               // lanes of a group, elements of a row per lane (the layout of bpr_device.h)
  int block;              // threads of a workgroup
  int groups_per_block;
  int pf;                 // prefetch depth of this (G, E): halved per doubling of E past 4 (the ring lives in VGPRs)
  int64_t groups;         // groups that take tickets: min(n, what the grid cap holds)
  int64_t grid;           // workgroups
};

// the same (G, E) as bpr_bind_tables chooses for a table of this d
inline void foldin_ge(int d, int* G, int* E) {
  const GroupShape g = group_shape(d);
  *G = g.G;
  *E = g.E;
}

// depth `base` at E <= 4, halved per doubling of E past 4: the rings live in VGPRs
constexpr int foldin_pf_at(int base, int E) { return E <= 4 ? base : std::max(1, base * 4 / E); }
constexpr int foldin_pf(int E) { return foldin_pf_at(FOLDIN_PF, E); }
constexpr int foldin_items_pf(int E) { return foldin_pf_at(BPR_FOLDIN_ITEMS_PF, E); }

// groups that take tickets and the workgroups that hold them: never more groups than rows, nor than `resident`
// workgroups on each of `cus` CUs hold at once
inline void foldin_groups_grid(int64_t n, int cus, int resident, int groups_per_block, int64_t* groups,
                               int64_t* grid) {
  const int64_t cap = (int64_t)std::max(cus, 1) * resident * groups_per_block;
  *groups = std::min<int64_t>(n, cap);
  *grid = (*groups + groups_per_block - 1) / groups_per_block;
}

// n >= 0, 1 <= d <= FOLDIN_MAX_D (checked by the callers)
inline FoldinPlan plan_foldin(int64_t n, int d, int cus = FOLDIN_CUS) {
  FoldinPlan p = {};
  foldin_ge(d, &p.G, &p.E);
  p.block = FOLDIN_BLOCK;
  p.groups_per_block = FOLDIN_BLOCK / p.G;
  p.pf = foldin_pf(p.E);
  foldin_groups_grid(n, cus, FOLDIN_RESIDENT, p.groups_per_block, &p.groups, &p.grid);
  return p;
}

}  // namespace bpr
