// bpr_warp.hip — the WARP objective (bpr_warp.h) in a translation unit of its own, as bpr_dynamic.hip holds the
// dynamic sampler: the k_stream<..., NEG_WARP, ...> instantiations (the group widths and "seen?" structures the
// launcher instantiates for the uniform sampler, plain kernel only), the stand-alone kernel k_sample_warp and the two
// entry points bpr_set_warp / bpr_sample_warp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "bpr_host.h"
#include "bpr_stream.h"
#include "bpr_warp_plan.h"

namespace bpr {

static_assert(NEG_WARP == BPR_NEG_WARP, "the kernels' template argument is the ABI's sampler kind");

// ---- the fused path: which k_stream a STREAM launch with BPR_NEG_WARP runs (launch_stream, bprcore.hip) ---------
template <int G, int E, int SN>
static StreamKernelFn warp_kernel_of(bool full) {
  return full ? &k_stream<G, E, NEG_WARP, SN, true> : &k_stream<G, E, NEG_WARP, SN, false>;
}

int stream_kernel_warp(const bpr_ctx* c, int seen, StreamKernelFn* out) {
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    const bool full = c->d == G * E;
    *out = seen == SEEN_BITMAP ? warp_kernel_of<G, E, SEEN_BITMAP>(full)
           : seen == SEEN_LIST ? warp_kernel_of<G, E, SEEN_LIST>(full)
                               : warp_kernel_of<G, E, SEEN_CSR>(full);
    return BPR_OK;
  });
}

// ---- the stand-alone kernel: one draw per (user, positive), on the tables as they are -------------------------
struct WarpArgs {
  const float* P;
  const float* Q;
  const float* bias;  // the ctx's dense item_bias, or NULL
  int64_t I;
  int d;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* users;
  const int32_t* pos;
  int64_t n;
  uint64_t seed, offset;
  int32_t N;
  float margin;
  int32_t* neg;
  int32_t* tries;
  float* x_pos;  // or NULL
  float* x_neg;  // or NULL
  ItemWeights iw;
};

// A group per draw, grid-stride; the "seen?" answer is the binary search of the CSR slice, as k_sample_dynamic's.
template <int G, int E>
__global__ __launch_bounds__(256) void k_sample_warp(const WarpArgs a) {
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
    const int32_t i = a.pos[tt];
    const int64_t lo = a.indptr[u], hi = a.indptr[u + 1];
    const SeenCsr seen{a.indices, lo, hi};
    float p[E], qi[E], q[E];
    load_row<G, E>(p, a.P + (int64_t)u * a.d, a.d, gl);
    const WarpPick w = sample_warp<G, E>(qi, q, p, rows, i, seen, hi - lo, a.indices + lo, a.I, a.seed,
                                         a.offset + (uint64_t)tt, a.N, a.margin, lane, a.iw);
    if (act && gl == 0) {
      a.neg[t] = w.item;
      a.tries[t] = w.tries;
      if (a.x_pos != nullptr) a.x_pos[t] = w.x_pos;
      if (a.x_neg != nullptr) a.x_neg[t] = w.x_neg;
    }
  }
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
  const char* who = "bpr_sample_warp";
  // the arguments first (the plan: plain numbers), then whatever touches the device
  if (c == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": ctx is NULL");
  if (c->P == nullptr || c->Q == nullptr)
    return fail(BPR_ERR_INVALID, std::string(who) + ": tables not bound (bpr_bind_tables)");
  WarpShape s = {};
  s.B = n; s.I = c->I; s.d = c->d; s.max_sampled = max_sampled; s.margin = margin;
  s.have_users = users != nullptr; s.have_pos = pos != nullptr;
  s.have_neg = neg_out != nullptr; s.have_tries = tries_out != nullptr; s.have_seen = c->indptr != nullptr;
  const WarpPlan p = plan_warp(s);
  if (p.rc != BPR_OK) return fail(p.rc, std::string(who) + ": " + p.why);
  if (p.G != c->G || p.E != c->E) return fail(BPR_ERR_INVALID, std::string(who) + ": group shape out of step");
  if (int rc = check_bound(c, who)) return rc;  // (folds hot deltas an asynchronous cut left: the table whole)
  if (p.grid == 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;  // reads the live rows
  WarpArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P; a.Q = c->Q; a.bias = c->bias; a.I = c->I; a.d = c->d;
  a.indptr = c->indptr; a.indices = c->indices;
  a.users = users; a.pos = pos; a.n = n; a.seed = seed; a.offset = offset;
  a.N = max_sampled; a.margin = margin;
  a.neg = neg_out; a.tries = tries_out; a.x_pos = xpos_out; a.x_neg = xneg_out;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_sample_warp<T::G, T::E>), dim3(p.grid), dim3(p.block), 0, c->stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

}  // extern "C"
