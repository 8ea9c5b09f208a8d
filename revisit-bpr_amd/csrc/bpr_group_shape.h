// bpr_group_shape.h — the rule from an embedding width d to the (G, E) group layout of bpr_device.h.  Plain C++17, no
// HIP: bpr_bind_tables (bprcore.hip) gives it to the ctx, and the plans that lay a launch out for a width without a
// ctx (bpr_scored_plan.h, bpr_foldin_plan.h) use the same function, so their kernels reduce a row in the order
// k_stream does.
#pragma once

namespace bpr {

// G lanes per triple and E row elements per lane of an embedding width d in [1, 1024]
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

}  // namespace bpr
