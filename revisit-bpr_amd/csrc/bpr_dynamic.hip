// bpr_dynamic.hip — dynamic negative sampling (bpr_scored.h) in a translation unit of its own, so that it compiles
// beside bpr_stream_launch.hip and leaves that file's kernels alone: the k_stream<..., NEG_DYNAMIC, ...> instantiations (the
// group widths and "seen?" structures the launcher instantiates for the uniform sampler, plain kernel only) and the
// two entry points bpr_set_dynamic / bpr_sample_dynamic — and, for both scored kinds, the stand-alone kernel
// k_sample_scored with its launcher (bpr_warp.hip calls it).
#include <hip/hip_runtime.h>

#include <string>

#include "bpr_host.h"
#include "bpr_stream.h"

namespace bpr {

// ---- the fused path: which k_stream a STREAM launch with BPR_NEG_DYNAMIC runs (launch_stream, bpr_stream_launch.hip)
int stream_kernel_dynamic(const bpr_ctx* c, int seen, StreamKernelFn* out) {
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    *out = stream_kernel_seen<T::G, T::E, NEG_DYNAMIC>(seen, c->d);
    return BPR_OK;
  });
}

// ---- the stand-alone kernel ---------------------------------------------------------------------------------------
// A group per draw, grid-stride; the "seen?" answer is the binary search of the CSR slice, as the stand-alone
// uniform kernel's (a draw tests a round or two of candidates).  Args: ScoredArgs (NEG_DYNAMIC) or ScoredWarpArgs
// (NEG_WARP) — a template argument of its own, so that the kernel's name holds no expression over KIND: the host and
// the device pass number the sampler kinds' unnamed enum differently, and a launch would not find its kernel.
template <int G, int E, int KIND, typename Args>
__global__ __launch_bounds__(256) void k_sample_scored(const Args a) {
  constexpr int GPW = 64 / G;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int gw = lane / G;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const TableRows<G, E> rows{a.Q, a.bias, a.d};
  for (int64_t base = wave * GPW; base < a.n; base += n_waves * GPW) {
    const int64_t t = base + gw;
    const bool act = t < a.n;
    const int64_t tt = act ? t : a.n - 1;
    const int32_t u = a.users[tt];
    int32_t i = 0;
    if constexpr (KIND == NEG_WARP) i = a.pos[tt];
    const int64_t lo = a.indptr[u], hi = a.indptr[u + 1];
    const SeenCsr seen{a.indices, lo, hi};
    float p[E], qi[E], q[E];
    load_row<G, E>(p, a.P + (int64_t)u * a.d, a.d, gl);
    const ScoredPick s = sample_scored<G, E, KIND>(qi, q, p, rows, i, seen, hi - lo, a.indices + lo, a.I, a.seed,
                                                   a.offset + (uint64_t)tt, a.K, a.margin, lane, a.iw);
    if (act && gl == 0) {
      a.neg[t] = s.item;
      if constexpr (KIND == NEG_WARP) {
        a.tries[t] = s.tries;
        if (a.x_pos != nullptr) a.x_pos[t] = s.x_pos;
      }
      if (a.x_neg != nullptr) a.x_neg[t] = s.x_neg;
    }
  }
}

// The arguments first (the plan: plain numbers), then whatever touches the device.  The caller has filled the call's
// part of the shape and of the arguments; the ctx's part is filled here.
int launch_sample_scored(bpr_ctx* c, const char* who, ScoredShape s, ScoredWarpArgs a) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": ctx is NULL");
  if (c->P == nullptr || c->Q == nullptr)
    return fail(BPR_ERR_INVALID, std::string(who) + ": tables not bound (bpr_bind_tables)");
  s.I = c->I; s.d = c->d; s.have_seen = c->indptr != nullptr;
  const ScoredPlan p = plan_scored(s);
  if (p.rc != BPR_OK) return fail(p.rc, std::string(who) + ": " + p.why);
  if (p.G != c->G || p.E != c->E) return fail(BPR_ERR_INVALID, std::string(who) + ": group shape out of step");
  if (int rc = check_bound(c, who)) return rc;  // (folds hot deltas an asynchronous cut left: the table whole)
  if (p.grid == 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;  // reads the live rows
  a.P = c->P; a.Q = c->Q; a.bias = c->bias; a.I = c->I; a.d = c->d;
  a.indptr = c->indptr; a.indices = c->indices;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using T = decltype(tag);
    if (s.kind == BPR_NEG_WARP)
      hipLaunchKernelGGL((k_sample_scored<T::G, T::E, NEG_WARP, ScoredWarpArgs>), dim3(p.grid), dim3(p.block), 0, c->stream, a);
    else
      hipLaunchKernelGGL((k_sample_scored<T::G, T::E, NEG_DYNAMIC, ScoredArgs>), dim3(p.grid), dim3(p.block), 0, c->stream,
                         static_cast<const ScoredArgs&>(a));
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

}  // namespace bpr

using namespace bpr;

extern "C" {

int bpr_set_dynamic(bpr_ctx* c, int32_t candidates) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_dynamic: ctx is NULL");
  if (!dynamic_candidates_ok(candidates))
    return fail(BPR_ERR_INVALID, "bpr_set_dynamic: candidates must be in [1, 32]");
  c->dyn_M = candidates;
  return BPR_OK;
}

int bpr_sample_dynamic(bpr_ctx* c, const int32_t* users, int64_t B, int32_t candidates, uint64_t seed,
                       uint64_t offset, int32_t* neg_out, float* score_out) {
  ScoredShape s = {};
  s.kind = BPR_NEG_DYNAMIC; s.B = B; s.count = candidates;
  s.have_users = users != nullptr; s.have_neg = neg_out != nullptr;
  ScoredWarpArgs a = {};
  a.users = users; a.n = B; a.seed = seed; a.offset = offset; a.K = candidates;
  a.neg = neg_out; a.x_neg = score_out;
  return launch_sample_scored(c, "bpr_sample_dynamic", s, a);
}

}  // extern "C"
