// bpr_strict.hip — the STRICT path: gradient scratch, k_triples / k_apply launches, the lazy-replay flush.
#include <string.h>

#include "bpr_ctx_state.h"
#include "bpr_host.h"
#include "bpr_kernels.h"
#include "bpr_opt_plan.h"

namespace bpr {

static int ensure_strict_scratch(bpr_ctx* c) {
  if (c->GP != nullptr) return BPR_OK;
  const size_t nP = (size_t)c->U * c->d, nQ = (size_t)c->I * c->d;
  BPR_HIP_CHECK(hipMalloc(&c->GP, sizeof(float) * nP));
  BPR_HIP_CHECK(hipMalloc(&c->GQ, sizeof(float) * nQ));
  BPR_HIP_CHECK(hipMalloc(&c->Gb, sizeof(float) * c->I));
  BPR_HIP_CHECK(hipMalloc(&c->flagP, sizeof(int32_t) * c->U));
  BPR_HIP_CHECK(hipMalloc(&c->flagQ, sizeof(int32_t) * c->I));
  BPR_HIP_CHECK(hipMalloc(&c->lastP, sizeof(int32_t) * c->U));
  BPR_HIP_CHECK(hipMalloc(&c->lastQ, sizeof(int32_t) * c->I));
  BPR_HIP_CHECK(hipMalloc(&c->touched, sizeof(uint32_t) * (size_t)(c->U + c->I)));
  BPR_HIP_CHECK(hipMalloc(&c->touched_cnt, 2 * sizeof(uint32_t)));
  BPR_HIP_CHECK(hipMemsetAsync(c->GP, 0, sizeof(float) * nP, c->stream));
  BPR_HIP_CHECK(hipMemsetAsync(c->GQ, 0, sizeof(float) * nQ, c->stream));
  BPR_HIP_CHECK(hipMemsetAsync(c->Gb, 0, sizeof(float) * c->I, c->stream));
  BPR_HIP_CHECK(hipMemsetAsync(c->flagP, 0, sizeof(int32_t) * c->U, c->stream));
  BPR_HIP_CHECK(hipMemsetAsync(c->flagQ, 0, sizeof(int32_t) * c->I, c->stream));
  // rows are current as of the step counter (0, or a resumed checkpoint's: bpr_set_step)
  BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastP, (int)c->step, (size_t)c->U, c->stream));
  BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastQ, (int)c->step, (size_t)c->I, c->stream));
  BPR_HIP_CHECK(hipMemsetAsync(c->touched_cnt, 0, 2 * sizeof(uint32_t), c->stream));
  c->cnt_sel = 0;
  c->pending = 0;
  return BPR_OK;
}

void free_strict_scratch(bpr_ctx* c) {
  hipFree(c->GP); hipFree(c->GQ); hipFree(c->Gb);
  hipFree(c->flagP); hipFree(c->flagQ); hipFree(c->lastP); hipFree(c->lastQ);
  hipFree(c->touched); hipFree(c->touched_cnt);
  c->GP = c->GQ = c->Gb = nullptr;
  c->flagP = c->flagQ = c->lastP = c->lastQ = nullptr;
  c->touched = c->touched_cnt = nullptr;
  c->pending = 0;
}

// the arguments of bpr_forward / bpr_forward_grad: the ctx's tables and scratch, and the call's batch and outputs
static TripleArgs triple_args(const bpr_ctx* c, const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t B,
                              float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  TripleArgs a;
  memset(&a, 0, sizeof(a));
  a.users = users; a.pos = pos; a.neg = neg; a.n = B;
  a.lpos = out_logits_pos; a.lneg = out_logits_neg; a.scalars = out_scalars;
  a.P = c->P; a.Q = c->Q; a.bias = c->bias;
  a.I = c->I; a.d = c->d;
  a.pad_user = c->pad_user; a.pad_item = c->pad_item;
  a.au = c->au; a.ai = c->ai; a.an = c->an;
  a.GP = c->GP; a.GQ = c->GQ; a.Gb = c->Gb;
  a.flagP = c->flagP; a.flagQ = c->flagQ;
  a.touched = c->touched; a.touched_cnt = c->touched_cnt + c->cnt_sel;
  a.partials = c->dev_scalars;
  a.acc_partials = c->defer_stats ? 1 : 0;
  a.mP = c->mP; a.vP = c->vP; a.mQ = c->mQ; a.vQ = c->vQ; a.mb = c->mb; a.vb = c->vb;
  // (Adagrad: no zero-gradient motion to read rows through — the kernel skips the block, as for SGD)
  if (opt_kind_lazy(c->opt_kind)) {
    a.lastP = c->lastP; a.lastQ = c->lastQ;
  }
  a.o = opt_dev(c, c->step + 1);
  return a;
}

static ApplyArgs apply_args(const bpr_ctx* c, int64_t t) {
  ApplyArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P; a.Q = c->Q; a.bias = c->bias;
  a.GP = c->GP; a.GQ = c->GQ; a.Gb = c->Gb;
  a.mP = c->mP; a.vP = c->vP; a.mQ = c->mQ; a.vQ = c->vQ; a.mb = c->mb; a.vb = c->vb;
  a.lastP = c->lastP; a.lastQ = c->lastQ;
  a.flagP = c->flagP; a.flagQ = c->flagQ;
  a.touched = c->touched; a.touched_cnt = c->touched_cnt + c->cnt_sel;
  a.next_cnt = c->touched_cnt + (c->cnt_sel ^ 1);
  a.U = c->U; a.I = c->I; a.d = c->d;
  a.pad_user = c->pad_user; a.pad_item = c->pad_item;
  a.o = opt_dev(c, t);
  return a;
}

// ---- launches ---------------------------------------------------------------------------------
template <int MODE>
static int launch_triples(bpr_ctx* c, TripleArgs a, bool timed) {
  if (a.n <= 0) return BPR_OK;
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    const unsigned grid = grid_for(a.n, G, 0);
    Timer tm(c, timed);
    (void)tm;
    hipLaunchKernelGGL((k_triples<G, E, MODE>), dim3(grid), dim3(256), 0, c->stream, a);
    // (k_sum_partials is not a template: it lives in bpr_stream_launch.o, its other user, and is launched through it)
    if (a.scalars != nullptr) return sum_partials(c, a.partials, (int)grid, a.scalars);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

// k_apply or k_discard (APPLY = false): one thread group per touched row, then flip cnt_sel
template <bool APPLY>
static int launch_touched(bpr_ctx* c) {
  ApplyArgs a = apply_args(c, c->step);
  int rc = dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    const unsigned grid = (unsigned)((c->pending * T::G + 255) / 256);
    if constexpr (APPLY) hipLaunchKernelGGL((k_apply<T::G, T::E>), dim3(grid), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL((k_discard<T::G, T::E>), dim3(grid), dim3(256), 0, c->stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
  if (rc) return rc;
  c->cnt_sel ^= 1;  // the kernel cleared the other counter
  c->pending = 0;
  return BPR_OK;
}

enum { FLUSH_USERS = 1, FLUSH_ITEMS = 2 };

// STRICT lazy replay: bring every row of the tables in `which` to step c->step (rows tracked by lastP / lastQ)
static int strict_flush_rows(bpr_ctx* c, int which, const char* who) {
  // SGD and Adagrad: a dense zero-gradient step moves nothing — no kernel
  if (!opt_kind_lazy(c->opt_kind) || c->GP == nullptr || c->step == 0) return BPR_OK;
  bias_moved(c);
  if (int rc = check_opt_state(c, who)) return rc;
  // (accumulated gradients of a batch in flight are left alone: the flush only advances w / m / v
  // and the rows' last-step marks, bpr_apply then finds nothing left to replay)
  ApplyArgs a = apply_args(c, c->step);
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    if (which & FLUSH_USERS)
      hipLaunchKernelGGL((k_flush_lazy<T::G, T::E>), dim3(grid_for(c->U, T::G, 0)), dim3(256), 0, c->stream, a, 0);
    if (which & FLUSH_ITEMS)
      hipLaunchKernelGGL((k_flush_lazy<T::G, T::E>), dim3(grid_for(c->I, T::G, 0)), dim3(256), 0, c->stream, a, 1);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

int strict_flush_impl(bpr_ctx* c) { return strict_flush_rows(c, FLUSH_USERS | FLUSH_ITEMS, "bpr_flush_lazy"); }

}  // namespace bpr

using namespace bpr;
extern "C" {

// ---- hot path -----------------------------------------------------------------------------------
int bpr_forward(bpr_ctx* c, const int32_t* users, const int32_t* pos, const int32_t* neg,
                int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  if (int rc = check_triples(c, "bpr_forward", users, pos, B)) return rc;
  if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, "bpr_forward: neg is NULL");
  if (int rc = vs_leave(c)) return rc;
  const TripleArgs a = triple_args(c, users, pos, neg, B, out_logits_pos, out_logits_neg, out_scalars);
  return launch_triples<MODE_FORWARD>(c, a, false);
}

int bpr_forward_grad(bpr_ctx* c, const int32_t* users, const int32_t* pos, const int32_t* neg,
                     int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  if (int rc = check_triples(c, "bpr_forward_grad", users, pos, B)) return rc;
  if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, "bpr_forward_grad: neg is NULL");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;
  if (int rc = ensure_strict_scratch(c)) return rc;
  const TripleArgs a = triple_args(c, users, pos, neg, B, out_logits_pos, out_logits_neg, out_scalars);
  c->pending += 3 * B;
  if (c->pending > c->U + c->I) c->pending = c->U + c->I;
  return launch_triples<MODE_GRAD>(c, a, true);
}

int bpr_apply(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_apply")) return rc;
  items_moved(c);
  bias_moved(c);
  if (int rc = check_opt_state(c, "bpr_apply")) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = ensure_strict_scratch(c)) return rc;
  c->step += 1;
  return c->pending > 0 ? launch_touched<true>(c) : BPR_OK;
}

int bpr_discard_grad(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_discard_grad")) return rc;
  if (c->GP == nullptr || c->pending == 0) return BPR_OK;
  return launch_touched<false>(c);  // (gradients only: neither table moves)
}

int bpr_get_grad(bpr_ctx* c, float* gP, float* gQ, float* gbias) {
  if (int rc = check_bound(c, "bpr_get_grad")) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = ensure_strict_scratch(c)) return rc;
  if (gP)
    BPR_HIP_CHECK(hipMemcpyAsync(gP, c->GP, sizeof(float) * (size_t)c->U * c->d,
                                 hipMemcpyDeviceToDevice, c->stream));
  if (gQ)
    BPR_HIP_CHECK(hipMemcpyAsync(gQ, c->GQ, sizeof(float) * (size_t)c->I * c->d,
                                 hipMemcpyDeviceToDevice, c->stream));
  if (gbias)
    BPR_HIP_CHECK(hipMemcpyAsync(gbias, c->Gb, sizeof(float) * (size_t)c->I,
                                 hipMemcpyDeviceToDevice, c->stream));
  return BPR_OK;
}

int bpr_step(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg, int64_t B,
             int32_t mode, int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
             float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  if (mode == BPR_MODE_STRICT)  // (dynamic: draw with bpr_sample_dynamic, pass the picks as BPR_NEG_GIVEN)
    if (int rc = refuse_scored("bpr_step (STRICT mode)", sampler)) return rc;
  if (int rc = check_triples(c, "bpr_step", users, pos, B)) return rc;
  if (int rc = check_sampler(c, "bpr_step", sampler, adaptive_p, neg, B)) return rc;
  if (mode == BPR_MODE_STREAM) {
    if (out_logits_pos || out_logits_neg)
      return fail(BPR_ERR_UNSUPPORTED, "bpr_step: STREAM mode does not return logits");
    return bpr_train_stream(c, users, pos, neg, B, sampler, adaptive_p, seed, offset, 0,
                            out_scalars);
  }
  if (mode != BPR_MODE_STRICT) return fail(BPR_ERR_INVALID, "bpr_step: unknown mode");
  if (sampler != BPR_NEG_GIVEN) {
    if (neg == nullptr && B > 0)
      return fail(BPR_ERR_INVALID, "bpr_step: STRICT mode needs a neg buffer to sample into");
    int rc = sampler == BPR_NEG_UNIFORM
                 ? bpr_sample_uniform(c, users, B, seed, offset, neg)
                 : bpr_sample_adaptive(c, users, B, adaptive_p, seed, offset, neg, nullptr,
                                       nullptr);
    if (rc) return rc;
  }
  if (int rc = bpr_forward_grad(c, users, pos, neg, B, out_logits_pos, out_logits_neg,
                                out_scalars))
    return rc;
  return bpr_apply(c);
}

int bpr_train_strict(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg_scratch,
                     int64_t n, int64_t B, int32_t sampler, float adaptive_p, uint64_t seed,
                     uint64_t offset, int64_t refresh_every, float* out_scalars) {
  // (dynamic: draw each batch with bpr_sample_dynamic, step with BPR_NEG_GIVEN)
  if (int rc = refuse_scored("bpr_train_strict", sampler)) return rc;
  if (int rc = check_triples(c, "bpr_train_strict", users, pos, n)) return rc;
  if (B < 1) return fail(BPR_ERR_INVALID, "bpr_train_strict: B must be >= 1");
  if (int rc = check_sampler(c, "bpr_train_strict", sampler, adaptive_p, neg_scratch, n)) return rc;
  if (sampler != BPR_NEG_GIVEN && neg_scratch == nullptr && n > 0)
    return fail(BPR_ERR_INVALID, "bpr_train_strict: neg_scratch is NULL");
  // loss statistics: k_triples adds each batch's partial sums to the per-block scratch and ONE
  // k_sum_partials at the end adds them to out_scalars (instead of one extra launch per batch)
  const bool defer = out_scalars != nullptr && n > 0;
  const unsigned stat_blocks = grid_for(B < n ? B : n, c->G, 0);
  if (defer) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    BPR_HIP_CHECK(hipMemsetAsync(c->dev_scalars, 0, sizeof(float) * 4 * stat_blocks, c->stream));
    c->defer_stats = true;
  }
  // AdaptiveSampler.sample (neg_samplers.py:74-124): _iteration_cnt += 1; draw with the CURRENT
  // snapshot; if _iteration_cnt % every == 0: update_stats() — i.e. the snapshot is retaken after
  // the draws of that batch and BEFORE its optimizer step, and the counter lives as long as the
  // sampler (it is not reset at epoch boundaries): c->strict_iter carries it across calls.
  int rc = BPR_OK;
  for (int64_t lo = 0; lo < n && rc == BPR_OK; lo += B) {
    const int64_t b = n - lo < B ? n - lo : B;
    int32_t* neg = sampler == BPR_NEG_GIVEN ? neg_scratch + lo : neg_scratch;
    if (sampler == BPR_NEG_UNIFORM)
      rc = bpr_sample_uniform(c, users + lo, b, seed, offset + (uint64_t)lo, neg);
    else if (sampler == BPR_NEG_ADAPTIVE)
      rc = bpr_sample_adaptive(c, users + lo, b, adaptive_p, seed, offset + (uint64_t)lo, neg,
                               nullptr, nullptr);
    c->strict_iter += 1;
    if (rc == BPR_OK && refresh_every > 0 && c->strict_iter % refresh_every == 0) {
      rc = bpr_flush_lazy(c);
      if (rc == BPR_OK) rc = bpr_adaptive_refresh(c);
    }
    if (rc == BPR_OK)
      rc = bpr_forward_grad(c, users + lo, pos + lo, neg, b, nullptr, nullptr, nullptr);
    if (rc == BPR_OK) rc = bpr_apply(c);
  }
  c->defer_stats = false;
  if (rc != BPR_OK) return rc;
  return defer ? sum_partials(c, c->dev_scalars, (int)stat_blocks, out_scalars) : BPR_OK;
}

int bpr_flush_lazy(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_flush_lazy")) return rc;
  items_moved(c);  // (the bias: the flush below says so if a kernel actually runs — vs_flush, strict_flush_rows)
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active) return vs_flush(c, true, true);  // batched STREAM bookkeeping is live
  return strict_flush_impl(c);
}

int bpr_flush_items(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_flush_items")) return rc;
  items_moved(c);
  bias_moved(c);
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active) return vs_flush(c, false, true);
  return strict_flush_rows(c, FLUSH_ITEMS, "bpr_flush_items");
}

}  // extern "C"
