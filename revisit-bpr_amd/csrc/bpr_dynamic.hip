// bpr_dynamic.hip — dynamic negative sampling (bpr_dynamic.h) in a translation unit of its own, so that it compiles
// beside bprcore.hip and leaves that file's kernels alone: the k_stream<..., NEG_DYNAMIC, ...> instantiations (the
// group widths and "seen?" structures the launcher instantiates for the uniform sampler, plain kernel only), the
// stand-alone kernel k_sample_dynamic and the two entry points bpr_set_dynamic / bpr_sample_dynamic.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "bpr_dynamic_plan.h"
#include "bpr_host.h"
#include "bpr_stream.h"

namespace bpr {

static_assert(NEG_DYNAMIC == BPR_NEG_DYNAMIC, "the kernels' template argument is the ABI's sampler kind");

// ---- the fused path: which k_stream a STREAM launch with BPR_NEG_DYNAMIC runs (launch_stream, bprcore.hip) ------
template <int G, int E, int SN>
static StreamKernelFn dynamic_kernel_of(bool full) {
  return full ? &k_stream<G, E, NEG_DYNAMIC, SN, true> : &k_stream<G, E, NEG_DYNAMIC, SN, false>;
}

int stream_kernel_dynamic(const bpr_ctx* c, int seen, StreamKernelFn* out) {
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    const bool full = c->d == G * E;
    *out = seen == SEEN_BITMAP ? dynamic_kernel_of<G, E, SEEN_BITMAP>(full)
           : seen == SEEN_LIST ? dynamic_kernel_of<G, E, SEEN_LIST>(full)
                               : dynamic_kernel_of<G, E, SEEN_CSR>(full);
    return BPR_OK;
  });
}

// ---- the stand-alone kernel: one draw per entry of users, on the tables as they are ---------------------------
struct DynamicArgs {
  const float* P;
  const float* Q;
  const float* bias;  // the ctx's dense item_bias, or NULL
  int64_t I;
  int d;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* users;
  int64_t n;
  uint64_t seed, offset;
  int32_t M;
  int32_t* neg;
  float* score;  // or NULL
  ItemWeights iw;
};

// A group per draw, grid-stride; the "seen?" answer is the binary search of the CSR slice, as the stand-alone
// uniform kernel's (a draw tests a round or two of candidates).
template <int G, int E>
__global__ __launch_bounds__(256) void k_sample_dynamic(const DynamicArgs a) {
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
    const int64_t lo = a.indptr[u], hi = a.indptr[u + 1];
    const SeenCsr seen{a.indices, lo, hi};
    float p[E], q[E];
    load_row<G, E>(p, a.P + (int64_t)u * a.d, a.d, gl);
    const DynamicPick pick = sample_dynamic<G, E>(q, p, rows, seen, hi - lo, a.indices + lo, a.I, a.seed,
                                                  a.offset + (uint64_t)tt, a.M, lane, a.iw);
    if (act && gl == 0) {
      a.neg[t] = pick.item;
      if (a.score != nullptr) a.score[t] = pick.score;
    }
  }
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
  const char* who = "bpr_sample_dynamic";
  // the arguments first (the plan: plain integers), then whatever touches the device
  if (c == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": ctx is NULL");
  if (c->P == nullptr || c->Q == nullptr)
    return fail(BPR_ERR_INVALID, std::string(who) + ": tables not bound (bpr_bind_tables)");
  DynamicShape s = {};
  s.B = B; s.I = c->I; s.d = c->d; s.candidates = candidates;
  s.have_users = users != nullptr; s.have_out = neg_out != nullptr; s.have_seen = c->indptr != nullptr;
  const DynamicPlan p = plan_dynamic(s);
  if (p.rc != BPR_OK) return fail(p.rc, std::string(who) + ": " + p.why);
  if (p.G != c->G || p.E != c->E) return fail(BPR_ERR_INVALID, std::string(who) + ": group shape out of step");
  if (int rc = check_bound(c, who)) return rc;  // (folds hot deltas an asynchronous cut left: the table whole)
  if (p.grid == 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;  // reads the live rows
  DynamicArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P; a.Q = c->Q; a.bias = c->bias; a.I = c->I; a.d = c->d;
  a.indptr = c->indptr; a.indices = c->indices;
  a.users = users; a.n = B; a.seed = seed; a.offset = offset; a.M = candidates;
  a.neg = neg_out; a.score = score_out;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_sample_dynamic<T::G, T::E>), dim3(p.grid), dim3(p.block), 0, c->stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

}  // extern "C"
