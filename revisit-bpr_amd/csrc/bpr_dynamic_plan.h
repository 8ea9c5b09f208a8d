// bpr_dynamic_plan.h — dynamic negative sampling (bpr_dynamic.h): the argument checks of bpr_set_dynamic /
// bpr_sample_dynamic and the layout of the stand-alone kernel's launch.  Integer arithmetic on the shape only: no HIP,
// no bpr_ctx (plain C++17; tests/dynamic_plan_check.cpp pins it on the CPU under the host sanitizers).  What a STREAM
// launch with BPR_NEG_DYNAMIC looks like is bpr_stream_plan.h's business: the "seen?" structures of the uniform
// sampler, never the LDS tier.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/bprcore.h"

namespace bpr {

constexpr int DYNAMIC_MIN = 1;       // candidates scored per triple: 1 (= the uniform sampler) ...
constexpr int DYNAMIC_MAX = 32;      // ... to 32 (lane s of a group keeps candidate s: half a wave)
constexpr int DYNAMIC_DEFAULT = 4;   // bpr_ctx's value until bpr_set_dynamic
constexpr int64_t DYNAMIC_MAX_GRID = 256 * 8;  // blocks of 256 threads: 256 CUs x 8 resident (grid-stride beyond)

inline bool dynamic_candidates_ok(int64_t m) { return m >= DYNAMIC_MIN && m <= DYNAMIC_MAX; }

// G lanes per triple and E row elements per lane of an embedding width d in [1, 1024] (bpr_device.h): what
// bpr_bind_tables gives the ctx, so the stand-alone kernel reduces a score in the order k_stream does.
struct GroupShape {
  int G, E;
};
inline GroupShape group_shape(int d) {
  GroupShape g;
  g.G = d <= 128 ? 32 : 64;
  const int per_lane = (d + g.G - 1) / g.G;
  g.E = g.G == 32 ? (per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : 4) : (per_lane <= 4 ? 4 : per_lane <= 8 ? 8 : 16);
  return g;
}

// rows in flight per chunk of candidates (bpr_dynamic.h dynamic_inflight<E>)
inline int dynamic_inflight_rows(int E) { return E <= 4 ? 8 : (E <= 8 ? 4 : 2); }

struct DynamicShape {
  int64_t B, I;      // draws of the call, item rows
  int d;
  int64_t candidates;
  bool have_users, have_out, have_seen;  // users / neg_out non-NULL, a seen CSR bound
  int64_t grid_cap;  // blocks a grid may have (0: DYNAMIC_MAX_GRID)
};

struct DynamicPlan {
  int rc;           // BPR_OK, or why the call is refused (nothing is launched then)
  const char* why;
  int G, E;
  unsigned block, grid;  // grid 0: nothing to do (B == 0)
  int chunks;       // round trips of candidate rows per draw: ceil(candidates / rows in flight)
};

inline DynamicPlan plan_dynamic(const DynamicShape& s) {
  DynamicPlan p = {};
  p.rc = BPR_ERR_INVALID;
  if (!dynamic_candidates_ok(s.candidates)) {
    p.why = "candidates must be in [1, 32]";
    return p;
  }
  if (!s.have_seen) {
    p.why = "seen CSR not bound";
    return p;
  }
  if (s.B < 0 || !s.have_users || !s.have_out) {
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
  p.chunks = (int)((s.candidates + rows - 1) / rows);
  return p;
}

}  // namespace bpr
