// bpr_scored_plan.h — the scored samplers (bpr_scored.h: dynamic negatives and the WARP objective): the argument
// checks of bpr_set_dynamic / bpr_sample_dynamic / bpr_set_warp / bpr_sample_warp and the layout of the stand-alone
// kernel's launch.  Integer arithmetic on the shape only: no HIP, no bpr_ctx (plain C++17; tests/dynamic_plan_check.cpp
// and tests/warp_plan_check.cpp pin it on the CPU under the host sanitizers).  What a STREAM launch with one of the
// two kinds looks like is bpr_stream_plan.h's business: the "seen?" structures of the uniform sampler, never the LDS
// tier.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/bprcore.h"
#include "bpr_group_shape.h"

namespace bpr {

// the kinds that score candidate rows under the live model inside the draw: fused into the plain-SGD k_stream only
constexpr bool sampler_scored(int kind) { return kind == BPR_NEG_DYNAMIC || kind == BPR_NEG_WARP; }

constexpr int DYNAMIC_MIN = 1;       // candidates scored per triple: 1 (= the uniform sampler) ...
constexpr int DYNAMIC_MAX = 32;      // ... to 32 (lane s of a group keeps candidate s: half a wave)
constexpr int DYNAMIC_DEFAULT = 4;   // bpr_ctx's value until bpr_set_dynamic
constexpr int64_t DYNAMIC_MAX_GRID = 256 * 8;  // blocks of 256 threads: 256 CUs x 8 resident (grid-stride beyond)
constexpr int WARP_MIN = 1;       // candidates tried per triple at most: 1 ...
constexpr int WARP_MAX = 32;      // ... to 32 (the same lanes)
constexpr int WARP_DEFAULT = 10;  // bpr_ctx's value until bpr_set_warp: LightFM's max_sampled
constexpr float WARP_DEFAULT_MARGIN = 1.0f;
constexpr int64_t WARP_MAX_GRID = DYNAMIC_MAX_GRID;

inline bool dynamic_candidates_ok(int64_t m) { return m >= DYNAMIC_MIN && m <= DYNAMIC_MAX; }
inline bool warp_max_sampled_ok(int64_t n) { return n >= WARP_MIN && n <= WARP_MAX; }
inline bool warp_margin_ok(float m) { return std::isfinite(m) && m > 0.f; }

// Candidate rows in flight at once: the loads of a chunk of rows are all issued before the first of them is
// reduced.  8 rows at E <= 4 (d <= 256: M = 8 is one round trip, M = 32 four); wider rows keep the chunk at 32
// registers per lane.
constexpr int dynamic_inflight_rows(int E) { return E <= 4 ? 8 : (E <= 8 ? 4 : 2); }

struct ScoredShape {
  int kind;          // BPR_NEG_DYNAMIC or BPR_NEG_WARP
  int64_t B, I;      // draws of the call, item rows
  int d;
  int64_t count;     // candidates (dynamic) / max_sampled (WARP)
  float margin;      // WARP only
  bool have_users, have_neg, have_seen;  // users / neg_out non-NULL, a seen CSR bound
  bool have_pos, have_tries;             // WARP only: pos / tries_out non-NULL
  int64_t grid_cap;  // blocks a grid may have (0: DYNAMIC_MAX_GRID)
};

struct ScoredPlan {
  int rc;           // BPR_OK, or why the call is refused (nothing is launched then)
  const char* why;
  int G, E;
  unsigned block, grid;  // grid 0: nothing to do (B == 0)
  int chunks;       // round trips of candidate rows per draw (WARP: at most): ceil(count / rows in flight)
};

inline ScoredPlan plan_scored(const ScoredShape& s) {
  const bool warp = s.kind == BPR_NEG_WARP;
  ScoredPlan p = {};
  p.rc = BPR_ERR_INVALID;
  if (!(warp ? warp_max_sampled_ok(s.count) : dynamic_candidates_ok(s.count))) {
    p.why = warp ? "max_sampled must be in [1, 32]" : "candidates must be in [1, 32]";
    return p;
  }
  if (warp && !warp_margin_ok(s.margin)) {
    p.why = "margin must be finite and > 0";
    return p;
  }
  if (!s.have_seen) {
    p.why = "seen CSR not bound";
    return p;
  }
  if (s.B < 0 || !s.have_users || !s.have_neg || (warp && (!s.have_pos || !s.have_tries))) {
    p.why = "bad argument";
    return p;
  }
  if (s.d < 1 || s.d > 1024 || s.I < 2) {
    p.why = "tables out of range";
    return p;
  }
  p.rc = BPR_OK;
  p.why = "";
  const GroupShape g = group_shape(s.d);
  p.G = g.G;
  p.E = g.E;
  p.block = 256;
  const int64_t per_block = 256 / g.G;
  const int64_t cap = s.grid_cap > 0 ? std::min<int64_t>(s.grid_cap, DYNAMIC_MAX_GRID) : DYNAMIC_MAX_GRID;
  p.grid = (unsigned)std::min<int64_t>(cap, s.B / per_block + (s.B % per_block != 0));
  const int rows = dynamic_inflight_rows(g.E);
  p.chunks = (int)((s.count + rows - 1) / rows);
  return p;
}

}  // namespace bpr
