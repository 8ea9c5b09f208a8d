// bpr_warp_plan.h — the WARP objective (bpr_warp.h): the argument checks of bpr_set_warp / bpr_sample_warp and the
// layout of the stand-alone kernel's launch.  Integer arithmetic on the shape only: no HIP, no bpr_ctx (plain C++17;
// tests/warp_plan_check.cpp pins it on the CPU under the host sanitizers).  What a STREAM launch with BPR_NEG_WARP
// looks like is bpr_stream_plan.h's business: the "seen?" structures of the uniform sampler, never the LDS tier.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/bprcore.h"
#include "bpr_dynamic_plan.h"

namespace bpr {

constexpr int WARP_MIN = 1;       // candidates tried per triple at most: 1 ...
constexpr int WARP_MAX = 32;      // ... to 32 (lane s of a group keeps candidate s: half a wave)
constexpr int WARP_DEFAULT = 10;  // bpr_ctx's value until bpr_set_warp: LightFM's max_sampled
constexpr float WARP_DEFAULT_MARGIN = 1.0f;
constexpr int64_t WARP_MAX_GRID = DYNAMIC_MAX_GRID;

inline bool warp_max_sampled_ok(int64_t n) { return n >= WARP_MIN && n <= WARP_MAX; }
inline bool warp_margin_ok(float m) { return std::isfinite(m) && m > 0.f; }

struct WarpShape {
  int64_t B, I;  // draws of the call, item rows
  int d;
  int64_t max_sampled;
  float margin;
  bool have_users, have_pos, have_neg, have_tries, have_seen;  // the pointers non-NULL, a seen CSR bound
  int64_t grid_cap;  // blocks a grid may have (0: WARP_MAX_GRID)
};

struct WarpPlan {
  int rc;  // BPR_OK, or why the call is refused (nothing is launched then)
  const char* why;
  int G, E;
  unsigned block, grid;  // grid 0: nothing to do (B == 0)
  int chunks;            // round trips of candidate rows per draw at most: ceil(max_sampled / rows in flight)
};

inline WarpPlan plan_warp(const WarpShape& s) {
  WarpPlan p = {};
  p.rc = BPR_ERR_INVALID;
  if (!warp_max_sampled_ok(s.max_sampled)) {
    p.why = "max_sampled must be in [1, 32]";
    return p;
  }
  if (!warp_margin_ok(s.margin)) {
    p.why = "margin must be finite and > 0";
    return p;
  }
  if (!s.have_seen) {
    p.why = "seen CSR not bound";
    return p;
  }
  if (s.B < 0 || !s.have_users || !s.have_pos || !s.have_neg || !s.have_tries) {
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
  const int64_t cap = s.grid_cap > 0 ? std::min<int64_t>(s.grid_cap, WARP_MAX_GRID) : WARP_MAX_GRID;
  p.grid = (unsigned)std::min<int64_t>(cap, s.B / per_block + (s.B % per_block != 0));
  const int rows = dynamic_inflight_rows(g.E);
  p.chunks = (int)((s.max_sampled + rows - 1) / rows);
  return p;
}

}  // namespace bpr
