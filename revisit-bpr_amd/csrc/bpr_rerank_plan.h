// bpr_rerank_plan.h — how a fused candidate re-ranking launch (k_rerank, bpr_rerank.hip) is laid out: which team of
// threads owns a row, the tile of candidates it stages at a time, dynamic LDS and the grid.  Integer arithmetic on
// the shape only: no HIP (plain C++17; tests/test_rerank_cpu.py pins it on the CPU through `bpr_test_rerank_plan`
// and compiles it alone, under the host sanitizers, into a program of its own).
//
// A row (one user with a list of candidates) is owned by ONE team and is never split:
//   RERANK_WAVE  a wave of 64 lanes per row, 4 rows per workgroup of 256 threads, tiles of 64 candidates;
//   RERANK_WG    the whole workgroup of 256 threads per row, tiles of 256 candidates.
// Either way a thread owns the fmaf chain of one candidate of the tile, the team stages the tile's item rows through
// LDS RERANK_KC features at a time in padded [tile][RERANK_LD] chunks (k_topk's, bpr_topk_plan.h), holds P[u] whole
// in LDS (d rounded up to RERANK_KC floats) and keeps a buffer of k + tile (score, id, position) candidates: the k
// best of the last compaction plus whatever one tile can append at worst.  No workspace.
//
// The grid is one workgroup per group of rows (1 row, or 4) up to RERANK_GRID_MAX workgroups; past that a workgroup
// walks groups g, g + grid, ... .  The hardware hands workgroups out as CUs fall free, which is what skewed list
// lengths need, and no counter has to be zeroed.
//
// What is marked NOT MEASURED rests on reasoning only; profiles/rerank_probe.txt and rerank_probe_rows.txt hold what
// the two layouts cost at the probe's shapes and are the place to start when moving a constant.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bpr_topk_plan.h"

namespace bpr {

constexpr int RERANK_AUTO = 0, RERANK_WAVE = 1, RERANK_WG = 2;  // the `layout` argument; 0 = the plan chooses
constexpr int RERANK_LAYOUTS = 2;
constexpr int RERANK_THREADS = 256;                // threads of a workgroup, both layouts
constexpr int RERANK_TILE_WAVE = 64;               // candidates of a tile, one per lane
constexpr int RERANK_TILE_WG = 256;                // candidates of a tile, one per thread
constexpr int RERANK_TILE = RERANK_TILE_WG;        // the largest tile (what revisit_bpr.rerank.RERANK_TILE reports)
constexpr int RERANK_KC = TOPK_KC;                 // features of a staged chunk: k_topk's, whose zero tail the chain repeats
constexpr int RERANK_LD = TOPK_LD;                 // floats of a staged row
constexpr int RERANK_DMAX = 1024;                  // largest d
constexpr size_t RERANK_LDS_LIMIT = 163840;        // LDS of a CU (gfx950)
// Which layout the plan chooses rests on profiles/rerank_probe.txt and rerank_probe_rows.txt (ML-20M shape, d = 128,
// k = 10; C = 100, 1,000 and 20,108 candidates per row; n = 1 .. 10,000 rows).  A wave walks its row alone — no
// workgroup barrier, no three waves idle while one compacts — and wins once there are rows enough to fill the chip
// with waves; a workgroup finishes ONE long row four times sooner, which is what counts while rows are few:
//   C = 100     the wave layout is never slower (equal up to 512 rows, 1.6 to 3.2 times faster from 1,024);
//   C = 1,000   equal up to 512 rows, the wave layout 1.5 to 2.4 times faster from 1,024 rows on;
//   C = 20,108  the workgroup layout 2.5 to 3 times faster up to 512 rows, 1.3 times at 1,024, within 5 % at 2,048
//               and 4,096; the wave layout 1.1 times faster at 10,000.
// The cuts below lie between those points.  NOT MEASURED: where exactly between 128 and 1,000 and between 1,000 and
// 20,108 candidates, and between 4,096 and 10,000 rows, the better layout changes; any other d or k.
constexpr int64_t RERANK_WAVE_MAX_LEN = 128;    // lists this short: the wave layout whatever n
constexpr int64_t RERANK_WAVE_MID_LEN = 1024;   // lists this short: the wave layout from RERANK_WAVE_MID_ROWS rows
constexpr int64_t RERANK_WAVE_MID_ROWS = 1024;
constexpr int64_t RERANK_WAVE_ANY_ROWS = 8192;  // this many rows: the wave layout whatever the length
// NOT MEASURED.  Workgroups of the largest grid (2^20; HIP wants grid x block below 2^32).
constexpr int64_t RERANK_GRID_MAX = (int64_t)1 << 20;

struct RerankPlan {
  int layout;           // RERANK_WAVE or RERANK_WG
  int tile;             // candidates of a tile
  int rows_per_group;   // rows of a workgroup: 4 or 1
  int cap;              // candidates a row's buffer holds: k + tile
  int64_t groups;       // ceil(n / rows_per_group)
  int64_t grid;         // workgroups launched: min(groups, RERANK_GRID_MAX)
  size_t team_lds;      // dynamic LDS of one team
  size_t lds;           // dynamic LDS of the workgroup: team_lds * rows_per_group
};

inline int rerank_dpad(int d) { return (d + RERANK_KC - 1) / RERANK_KC * RERANK_KC; }

// one team: the staged tile, P[u], the tile's eligible ids, the candidate buffer of 12-byte entries, the threshold
// (12 bytes), count and pending count; rounded up to 16 bytes so that the next team's staging stays aligned
inline size_t rerank_team_lds(int tile, int d, int k) {
  const size_t b = sizeof(float) * (size_t)tile * RERANK_LD + sizeof(float) * (size_t)rerank_dpad(d) +
                   sizeof(int32_t) * (size_t)tile + (size_t)(k + tile) * 12 + 12 + 4 + 4;
  return (b + 15) / 16 * 16;
}
static_assert(RERANK_THREADS / 64 * (4 * (size_t)RERANK_TILE_WAVE * RERANK_LD + 4 * (size_t)RERANK_DMAX +
                                     4 * (size_t)RERANK_TILE_WAVE + (size_t)(TOPK_MAX + RERANK_TILE_WAVE) * 12 + 32) <=
                  65536,
              "the wave layout at the largest k and d must fit the 64 KiB a kernel gets without asking");
static_assert(4 * (size_t)RERANK_TILE_WG * RERANK_LD + 4 * (size_t)RERANK_DMAX + 4 * (size_t)RERANK_TILE_WG +
                      (size_t)(TOPK_MAX + RERANK_TILE_WG) * 12 + 32 <= 65536,
              "the workgroup layout at the largest k and d must fit the 64 KiB a kernel gets without asking");

// row_len: the length of the shared list, or the caller's hint of a typical CSR row (0 = unknown, taken as long:
// the plan cannot read the candidate indptr, which lives on the device)
inline int rerank_auto_layout(int64_t n, int64_t row_len) {
  if (row_len > 0 && row_len <= RERANK_WAVE_MAX_LEN) return RERANK_WAVE;
  if (row_len > 0 && row_len <= RERANK_WAVE_MID_LEN && n >= RERANK_WAVE_MID_ROWS) return RERANK_WAVE;
  return n >= RERANK_WAVE_ANY_ROWS ? RERANK_WAVE : RERANK_WG;
}

// n >= 0, 1 <= d <= RERANK_DMAX, 0 <= k <= TOPK_MAX, row_len >= 0, layout in {0, 1, 2} (checked by the callers)
inline RerankPlan plan_rerank(int64_t n, int d, int k, int64_t row_len, int layout) {
  RerankPlan p = {};
  p.layout = layout == RERANK_AUTO ? rerank_auto_layout(n, row_len) : layout;
  p.tile = p.layout == RERANK_WAVE ? RERANK_TILE_WAVE : RERANK_TILE_WG;
  p.rows_per_group = p.layout == RERANK_WAVE ? RERANK_THREADS / 64 : 1;
  p.cap = k + p.tile;
  p.groups = n / p.rows_per_group + (n % p.rows_per_group != 0);
  p.grid = std::min<int64_t>(p.groups, RERANK_GRID_MAX);
  p.team_lds = rerank_team_lds(p.tile, d, k);
  p.lds = p.team_lds * (size_t)p.rows_per_group;
  return p;
}

}  // namespace bpr
