// bpr_diversify_plan.h — how a fused MMR re-ranking launch (k_diversify, bpr_diversify.hip) is laid out: the padded
// pool, the tiles of the Gram matrix a row keeps in LDS, dynamic LDS and the grid.  Integer arithmetic on the shape
// only: no HIP (plain C++17; tests/test_diversify_cpu.py pins it on the CPU through `bpr_test_diversify_plan` and
// compiles it alone, under the host sanitizers, into a program of its own).
//
// A row (a pool of C <= DIVERSIFY_CMAX candidates) is owned by ONE workgroup of 256 threads and is never split.  The
// pool is padded to cpad, a multiple of 32, and cut into T = cpad / 32 tiles of 32 candidates.  The workgroup holds
//   the Gram matrix: only the T (T + 1) / 2 tiles (ti <= tj) on or above the diagonal, each a [32][DIVERSIFY_TILE_LD]
//     block of floats (the similarity is symmetric bit for bit, so the lower half is never computed and never stored;
//     33 floats a row so that a ROW of a tile and a COLUMN of a tile are both read by 32 lanes on 32 banks);
//   one staged chunk of the candidates' item rows, [cpad][DIVERSIFY_LD] floats (k_topk's padded chunk of 32 features);
//   per candidate its id, relevance and 1 / norm;
//   the exchange of the greedy phase: two waves x two parities of a 16-byte key, and the row's few scalars.
// Nothing depends on d or k.  At cpad = 128 that is 62,336 bytes: below the 64 KiB a kernel gets without asking, and
// two workgroups fit a CU; at cpad = 32 it is 9,344 bytes and at 64 22,784, so short pools leave room for many.
//
// The grid is one workgroup per row up to DIVERSIFY_GRID_MAX workgroups; past that a workgroup walks rows r,
// r + grid, ... (as k_rerank does).
//
// There is ONE layout today (a workgroup per row).  The `layout` argument exists so that a second one (a wave per row
// for pools of <= 32, several rows to a workgroup) can be forced when it is added; NOT MEASURED whether it would pay.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bpr_topk_plan.h"

namespace bpr {

constexpr int DIVERSIFY_AUTO = 0, DIVERSIFY_WG = 1;  // the `layout` argument; 0 = the plan chooses
constexpr int DIVERSIFY_LAYOUTS = 1;
constexpr int DIVERSIFY_THREADS = 256;               // threads of a workgroup
constexpr int DIVERSIFY_CMAX = TOPK_MAX;             // longest pool, and largest k: what recommend / rerank return
constexpr int DIVERSIFY_TILE = 32;                   // candidates of a Gram tile (v_mfma_f32_32x32x2_f32)
constexpr int DIVERSIFY_TILE_LD = DIVERSIFY_TILE + 1;  // floats of a stored tile row
constexpr int DIVERSIFY_KC = TOPK_KC;                // features of a staged chunk: k_topk's, whose zero tail the chain repeats
constexpr int DIVERSIFY_LD = TOPK_LD;                // floats of a staged row
constexpr int DIVERSIFY_DMAX = 1024;                 // largest d
constexpr size_t DIVERSIFY_LDS_LIMIT = 163840;       // LDS of a CU (gfx950)
constexpr int64_t DIVERSIFY_GRID_MAX = (int64_t)1 << 20;  // workgroups of the largest grid (HIP: grid x block < 2^32)

struct DiversifyPlan {
  int layout;      // DIVERSIFY_WG
  int cpad;        // the pool padded to a multiple of DIVERSIFY_TILE
  int tiles;       // Gram tiles held: T (T + 1) / 2, T = cpad / 32
  int64_t grid;    // workgroups launched: min(n, DIVERSIFY_GRID_MAX)
  size_t lds;      // dynamic LDS of the workgroup
};

constexpr int diversify_cpad(int C) { return (C + DIVERSIFY_TILE - 1) / DIVERSIFY_TILE * DIVERSIFY_TILE; }
constexpr int diversify_tiles(int cpad) { return (cpad / DIVERSIFY_TILE) * (cpad / DIVERSIFY_TILE + 1) / 2; }

// Gram tiles, the staged chunk, per candidate (id, relevance, 1 / norm), the greedy exchange (2 waves x 2 parities x
// 16 bytes) and 16 words of row scalars; every part is a multiple of 16 bytes
constexpr size_t diversify_lds_bytes(int cpad) {
  return sizeof(float) * (size_t)diversify_tiles(cpad) * DIVERSIFY_TILE * DIVERSIFY_TILE_LD +
         sizeof(float) * (size_t)cpad * DIVERSIFY_LD + 12 * (size_t)cpad + 64 + 64;
}
static_assert(diversify_lds_bytes(DIVERSIFY_CMAX) == 62336, "the C = 128 budget: 42,240 + 18,432 + 1,536 + 128");
static_assert(diversify_lds_bytes(DIVERSIFY_CMAX) <= 65536,
              "the longest pool must fit the 64 KiB a kernel gets without asking");
static_assert(2 * diversify_lds_bytes(DIVERSIFY_CMAX) <= DIVERSIFY_LDS_LIMIT,
              "two workgroups of the longest pool must fit the CU's 163,840 bytes");

// n >= 0, 1 <= C <= DIVERSIFY_CMAX, layout in {0, 1} (checked by the callers)
inline DiversifyPlan plan_diversify(int64_t n, int C, int layout) {
  DiversifyPlan p = {};
  p.layout = layout == DIVERSIFY_AUTO ? DIVERSIFY_WG : layout;
  p.cpad = diversify_cpad(C);
  p.tiles = diversify_tiles(p.cpad);
  p.grid = std::min<int64_t>(n, DIVERSIFY_GRID_MAX);
  p.lds = diversify_lds_bytes(p.cpad);
  return p;
}

}  // namespace bpr
