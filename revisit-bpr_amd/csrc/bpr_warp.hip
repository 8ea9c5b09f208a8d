// bpr_warp.hip — the WARP objective (bpr_scored.h) in a translation unit of its own, as bpr_dynamic.hip holds the
// dynamic sampler: the k_stream<..., NEG_WARP, ...> instantiations (the group widths and "seen?" structures the
// launcher instantiates for the uniform sampler, plain kernel only) and the two entry points bpr_set_warp /
// bpr_sample_warp (the stand-alone kernel and its launcher: bpr_dynamic.hip).
#include <hip/hip_runtime.h>

#include "bpr_host.h"
#include "bpr_stream.h"

namespace bpr {

// ---- the fused path: which k_stream a STREAM launch with BPR_NEG_WARP runs (launch_stream, bpr_stream_launch.hip)----
int stream_kernel_warp(const bpr_ctx* c, int seen, StreamKernelFn* out) {
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    *out = stream_kernel_seen<T::G, T::E, NEG_WARP>(seen, c->d);
    return BPR_OK;
  });
}

}  // namespace bpr

using namespace bpr;

extern "C" {

int bpr_set_warp(bpr_ctx* c, int32_t max_sampled, float margin) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_warp: ctx is NULL");
  if (!warp_max_sampled_ok(max_sampled))
    return fail(BPR_ERR_INVALID, "bpr_set_warp: max_sampled must be in [1, 32]");
  if (!warp_margin_ok(margin)) return fail(BPR_ERR_INVALID, "bpr_set_warp: margin must be finite and > 0");
  c->warp_N = max_sampled;
  c->warp_margin = margin;
  return BPR_OK;
}

int bpr_sample_warp(bpr_ctx* c, const int32_t* users, const int32_t* pos, int64_t n, int32_t max_sampled,
                    float margin, uint64_t seed, uint64_t offset, int32_t* neg_out, int32_t* tries_out,
                    float* xpos_out, float* xneg_out) {
  ScoredShape s = {};
  s.kind = BPR_NEG_WARP; s.B = n; s.count = max_sampled; s.margin = margin;
  s.have_users = users != nullptr; s.have_pos = pos != nullptr;
  s.have_neg = neg_out != nullptr; s.have_tries = tries_out != nullptr;
  ScoredWarpArgs a = {};
  a.users = users; a.pos = pos; a.n = n; a.seed = seed; a.offset = offset;
  a.K = max_sampled; a.margin = margin;
  a.neg = neg_out; a.tries = tries_out; a.x_pos = xpos_out; a.x_neg = xneg_out;
  return launch_sample_scored(c, "bpr_sample_warp", s, a);
}

}  // extern "C"
