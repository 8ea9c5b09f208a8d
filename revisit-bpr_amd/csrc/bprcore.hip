// bprcore.hip — C ABI of libbprcore.so (declared in include/bprcore.h) and kernel dispatch.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "bpr_ctx.h"
#include "bpr_kernels.h"
#include "bpr_host.h"
#include "bpr_stream_plan.h"
#include "bpr_refresh_plan.h"
#include "bpr_group_shape.h"
#include "bpr_opt_plan.h"

namespace bpr {
static_assert(ORDER_PAD == BPR_ORDER_PAD, "walk vector width vs snapshot padding");
static_assert(SEEN_CSR == STREAM_SEEN_CSR && SEEN_BITMAP == STREAM_SEEN_BITMAP && SEEN_LIST == STREAM_SEEN_LIST &&
                  NEG_GIVEN == BPR_NEG_GIVEN && NEG_DYNAMIC == BPR_NEG_DYNAMIC && NEG_WARP == BPR_NEG_WARP,
              "the launch plan names the kernels' template arguments");

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

static int max_blocks() {
  static int v = [] {
    const char* e = getenv("BPR_MAX_BLOCKS");
    int n = e ? atoi(e) : 0;
    return n > 0 ? n : 256 * 8;  // 256 CUs x 8 resident 256-thread blocks
  }();
  return v;
}
// STREAM grids (bpr_stream_plan.h): BPR_MAX_BLOCKS caps them (experiments).
static int64_t stream_grid_cap() {
  static const bool forced = getenv("BPR_MAX_BLOCKS") != nullptr;
  return forced ? (int64_t)max_blocks() : STREAM_MAX_GRID;
}

// grid for n groups of G lanes, 256-thread blocks, capped (grid-stride inside the kernels)
static unsigned grid_for(int64_t n_groups, int G, int64_t cap_groups) {
  if (cap_groups > 0 && n_groups > cap_groups) n_groups = cap_groups;
  const int64_t per_block = 256 / G;
  int64_t blocks = (n_groups + per_block - 1) / per_block;
  if (blocks > max_blocks()) blocks = max_blocks();
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

int check_bound(const bpr_ctx* c, const char* who, bool whole_table) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": ctx is NULL");
  if (c->P == nullptr || c->Q == nullptr)
    return fail(BPR_ERR_INVALID, std::string(who) + ": tables not bound (bpr_bind_tables)");
  // every entry point sees the item table whole — but bpr_train_stream_acut itself and the calls of
  // its pipeline that never look at the table (commit; begin when the keys are already cut)
  if (whole_table && c->hot_unfolded && !c->acut_call) return hot_fold_impl(const_cast<bpr_ctx*>(c));
  return BPR_OK;
}

// k_stream_epilogue: the sum of a launch's loss partials (out != NULL), the fold of the hot block into Q and the
// write-back of the wide item_bias, each if asked for.  `stop`: an event that rides on the kernel's own completion.
static int stream_epilogue(bpr_ctx* c, const float* partials, int n_blocks, float* out, bool fold, bool with_bias,
                           hipEvent_t stop) {
  EpilogueArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.partials = partials; ea.n_blocks = n_blocks; ea.out = out;
  ea.Q = c->Q; ea.delta = c->hot_delta; ea.hot_items = c->hot_items;
  ea.H = fold ? c->hot_H : 0; ea.R = c->hot_R; ea.d = c->d;
  ea.fold_blocks = fold ? (int)std::min<int64_t>(((int64_t)c->hot_H * c->d + 255) / 256, 64) : 0;
  if (with_bias) {
    ea.bias_w = c->bias_w; ea.bias = c->bias; ea.I = (int32_t)c->I;
    ea.bias_blocks = (int)std::min<int64_t>((c->I + 255) / 256, 256);
  }
  const dim3 grid(1 + ea.fold_blocks + ea.bias_blocks);
  if (stop != nullptr)
    hipExtLaunchKernelGGL(k_stream_epilogue, grid, dim3(256), 0, c->stream, nullptr, stop, 0, ea);
  else
    hipLaunchKernelGGL(k_stream_epilogue, grid, dim3(256), 0, c->stream, ea);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

// Fold the hot deltas an asynchronous cut left in the block (after that cut has read them).
int hot_fold_impl(bpr_ctx* c) {
  if (!c->hot_unfolded) return BPR_OK;
  c->hot_unfolded = false;
  if (c->hot_H <= 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->ev_keys != nullptr) BPR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_keys, 0));
  c->acut_pending = false;
  if (int rc = stream_epilogue(c, nullptr, 0, nullptr, true, false, nullptr)) return rc;
  return BPR_OK;  // (Q + delta is what it was: keys cut from it stay valid)
}

// bpr_train_stream_cut under the hot tier leaves its loss partials to the bpr_sync_cut that should
// follow.  Whoever comes first instead — the next launch (it overwrites the partials), a hot exchange
// of the three-call protocol (bpr_hot_exchange / bpr_hot_sync), the end of the tier — sums them now.
int flush_deferred_stats(bpr_ctx* c) {
  if (!c->defer_pending) return BPR_OK;
  c->defer_pending = false;
  float* out = c->defer_out;
  c->defer_out = nullptr;
  if (out == nullptr || c->defer_blocks <= 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->dev_scalars, c->defer_blocks, out);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

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

static void free_strict_scratch(bpr_ctx* c) {
  hipFree(c->GP); hipFree(c->GQ); hipFree(c->Gb);
  hipFree(c->flagP); hipFree(c->flagQ); hipFree(c->lastP); hipFree(c->lastQ);
  hipFree(c->touched); hipFree(c->touched_cnt);
  c->GP = c->GQ = c->Gb = nullptr;
  c->flagP = c->flagQ = c->lastP = c->lastQ = nullptr;
  c->touched = c->touched_cnt = nullptr;
  c->pending = 0;
}


static TripleArgs triple_args(const bpr_ctx* c) {
  TripleArgs a;
  memset(&a, 0, sizeof(a));
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

OptDev opt_dev(const bpr_ctx* c, int64_t t) {
  OptDev o;
  memset(&o, 0, sizeof(o));
  o.kind = c->opt_kind;
  o.lr = c->opt.lr; o.mu = c->opt.momentum; o.damp = c->opt.dampening;
  o.nesterov = c->opt.nesterov;
  o.b1 = c->opt.beta1; o.b2 = c->opt.beta2; o.eps = c->opt.eps; o.alpha = c->opt.alpha;
  o.t = t;
  auto safe_log = [](double x) { return x > 0.0 ? log(x) : -1.0e30; };
  o.log_b1 = safe_log((double)o.b1);
  o.log_b2 = safe_log((double)o.b2);
  o.log_mu = safe_log((double)o.mu);
  o.log_alpha = safe_log((double)o.alpha);
  // Adam replay: terms decay like (b1/sqrt(b2))^s; stop once below 1e-8 of the first
  o.kmax = 0;
  o.t_sat = -1;
  o.adam_step = 0.f;
  o.adam_bc2 = 1.f;
  if (o.kind == OPT_ADAM) {
    o.adam_step = (float)((double)o.lr / (1.0 - exp((double)t * o.log_b1)));
    o.adam_bc2 = (float)sqrt(1.0 - exp((double)t * o.log_b2));
  }
  if (o.kind == OPT_ADAGRAD) o.adam_step = adagrad_clr(c->opt.lr, c->opt.lr_decay, t);  // the step's clr
  if (o.kind == OPT_ADAM && o.b1 > 0.f) {
    const double ratio = (double)o.b1 / sqrt((double)o.b2);
    o.kmax = ratio < 1.0 ? (int)ceil(log(1e-8) / log(ratio)) : 1 << 20;
    // closed-form replay (bpr_kernels.h: opt_replay_row): needs 1 - b^t to round to 1.0f for every
    // replayed t (b^t < 2^-25) and all three series ratios b1 / b2^((j+1)/2) below 1
    const bool no_closed = c->tune_adam_closed == 0;  // bpr_set_tuning("adam_closed", 0): tests compare both routes
    const double zmax = (double)o.b1 / pow((double)o.b2, 0.5 * ADAM_SERIES);
    if (!no_closed && zmax < 0.999 && o.b1 < 1.f && o.b2 > 0.f && o.b2 < 1.f) {
      const double lim = log(ldexp(1.0, -25));
      const double t1 = ceil(lim / log((double)o.b1)), t2 = ceil(lim / log((double)o.b2));
      o.t_sat = (int64_t)(t1 > t2 ? t1 : t2);  // replayed steps are s0+1 .. : s0 >= t_sat suffices
      o.sv_min = (float)((double)o.eps * pow((double)o.b2, -0.5 * o.kmax) / 0.2);
      for (int j = 0; j < ADAM_SERIES; ++j) {
        const double lz = log((double)o.b1) - 0.5 * (j + 1) * log((double)o.b2), z = exp(lz);
        o.G[j] = (float)(z * (1.0 - exp((double)o.kmax * lz)) / (1.0 - z));
        o.log2_z[j] = (float)(lz / log(2.0));
        o.zc[j] = (float)(z / (1.0 - z));
      }
    }
  }
  return o;
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

int check_opt_state(const bpr_ctx* c, const char* who) {
  const bool need_m = c->opt_kind == BPR_OPT_MOMENTUM || c->opt_kind == BPR_OPT_ADAM ||
                      (c->opt_kind == BPR_OPT_RMSPROP && c->opt.momentum > 0.f);
  const bool need_v = c->opt_kind == BPR_OPT_ADAM || c->opt_kind == BPR_OPT_RMSPROP ||
                      c->opt_kind == BPR_OPT_ADAGRAD;  // (Adagrad: v = sum, no m)
  if ((need_m && (!c->mP || !c->mQ || (c->bias && !c->mb))) ||
      (need_v && (!c->vP || !c->vQ || (c->bias && !c->vb))))
    return fail(BPR_ERR_INVALID,
                std::string(who) + ": optimizer state not bound (bpr_bind_opt_state)");
  return BPR_OK;
}

static int drain_timing(bpr_ctx* c) {
  if (c->ev_used == 0) return BPR_OK;
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < c->ev_used; ++k) {
    float ms = 0.f;
    BPR_HIP_CHECK(hipEventElapsedTime(&ms, c->ev_start[k], c->ev_stop[k]));
    c->timed_ms += (double)ms;
    c->timed_launches += 1;
  }
  c->ev_used = 0;
  return BPR_OK;
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
    if (a.scalars != nullptr)
      hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, a.partials, (int)grid,
                         a.scalars);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

// CUs the ctx's launch stream may use: the popcount of its CU mask (bpr_stream_create), the whole
// chip for an unmasked stream.  Queried once per stream handle.
static int stream_cus(bpr_ctx* c) {
  if (c->stream_cus_of == (void*)c->stream && c->stream_cus > 0) return c->stream_cus;
  int n_cu = 0;
  hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  int cus = n_cu;
  if (c->stream != nullptr) {
    uint32_t mask[16] = {0};
    if (hipExtStreamGetCUMask(c->stream, 16, mask) == hipSuccess) {
      int bits = 0;
      for (int w = 0; w < 16; ++w) bits += __builtin_popcount(mask[w]);
      if (bits > 0 && bits < n_cu) cus = bits;
    } else {
      (void)hipGetLastError();
    }
  }
  c->stream_cus = cus > 0 ? cus : 256;
  c->stream_cus_of = (void*)c->stream;
  return c->stream_cus;
}

// ---- STREAM ------------------------------------------------------------------------------------
// the plain k_stream instantiation for the ctx's shape (the LDSHOT ones: bpr_hotlds.hip)
static int stream_kernel(const bpr_ctx* c, int sampler, int seen, bool part, StreamKernelFn* out) {
  if (sampler == NEG_DYNAMIC) return stream_kernel_dynamic(c, seen, out);  // (bpr_dynamic.hip)
  if (sampler == NEG_WARP) return stream_kernel_warp(c, seen, out);        // (bpr_warp.hip)
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    *out = sampler == NEG_GIVEN     ? stream_kernel_of<G, E, NEG_GIVEN, SEEN_CSR>(c->d == G * E, false)
           : sampler == NEG_UNIFORM ? stream_kernel_seen<G, E, NEG_UNIFORM>(seen, c->d)
                                    : stream_kernel_seen<G, E, NEG_ADAPTIVE>(seen, c->d, part);
    return BPR_OK;
  });
}

// blocks of the plan's plain kernel a CU holds at once (asked of the instantiation for a snapshot sorted whole),
// cached per (d, sampler, seen, block, shmem) until the next bpr_set_tuning
static int stream_occupancy(bpr_ctx* c, int sampler, const StreamPlan& p, int* occ) {
  const auto key = std::make_tuple(c->d, sampler, p.seen, (int)p.block, (int64_t)p.shmem);
  const auto it = c->stream_occ.find(key);
  if (it != c->stream_occ.end()) {
    *occ = it->second;
    return BPR_OK;
  }
  StreamKernelFn k = nullptr;
  if (int rc = stream_kernel(c, sampler, p.seen, false, &k)) return rc;
  *occ = 0;
  hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k, (int)p.block, p.shmem);
  if (*occ < 1) {
    (void)hipGetLastError();
    *occ = 1;
  }
  c->stream_occ[key] = *occ;
  return BPR_OK;
}

// k_stream_epilogue_cut / k_sync_cut: the cut of the next snapshot's keys (Q + the hot block, transposed into
// c->keysT) with the sum of the loss partials; fold: the hot block is folded into Q on the way; hot = false: the
// keys are Q alone
static EpilogueCutArgs cut_args(const bpr_ctx* c, const float* partials, int n_blocks, float* out, bool hot, bool fold,
                                bool with_bias) {
  EpilogueCutArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.partials = partials; ea.n_blocks = n_blocks; ea.out = out;
  ea.Q = c->Q; ea.T = c->keysT; ea.sig_acc = c->sig_acc; ea.d = c->d; ea.I = (int32_t)c->I;
  if (hot) { ea.delta = c->hot_delta; ea.hot_slot = c->hot_slot; ea.H = c->hot_H; ea.R = c->hot_R; }
  ea.fold = fold ? 1 : 0;
  if (with_bias) { ea.bias_w = c->bias_w; ea.bias = c->bias; }
  return ea;
}
static dim3 cut_grid(const bpr_ctx* c) { return dim3((unsigned)((c->I + 31) / 32), (unsigned)((c->d + 31) / 32) + 1u); }

static int ensure_cut_events(bpr_ctx* c) {
  if (c->ev_keys != nullptr) return BPR_OK;
  BPR_HIP_CHECK(hipEventCreateWithFlags(&c->ev_keys, hipEventDisableTiming));
  BPR_HIP_CHECK(hipEventCreateWithFlags(&c->ev_sorted, hipEventDisableTiming));
  return BPR_OK;
}

// c->keysT holds the next snapshot's keys: the next bpr_adaptive_refresh_begin only queues the sort.  by_event:
// ev_keys rides on the cut kernel; on_side: the cut runs on c->side — whoever sorts these keys on the launch stream
// waits for ev_keys, and so does a launch outside the acut pipeline (the cut reads Q and that launch's partials)
static void mark_keys_cut(bpr_ctx* c, bool by_event, bool on_side) {
  c->keys_cut = true;
  if (c->meta_front != nullptr && c->keysT == c->keys_front) c->keys_front_stale = true;
  c->keys_event = by_event;
  if (on_side) c->keys_on_side = c->acut_pending = true;
}

// One STREAM launch: one group per run of run_len triples; max_inflight (cap_groups) caps the number of groups
// (= triples in flight).  The layout of the launch is decided in bpr_stream_plan.h.
static int launch_stream(bpr_ctx* c, StreamArgs a, int sampler, int64_t cap_groups,
                         float* out_scalars, bool cut, bool acut = false) {
  if (a.n <= 0) return BPR_OK;
  if (cut)
    if (int rc = refresh_alloc(c)) return rc;
  if (int rc = flush_deferred_stats(c)) return rc;  // (this launch overwrites the partials)
  if (c->acut_pending && !acut) {
    // the asynchronous cut of the previous launch still reads that launch's partials (and Q + the hot
    // deltas) on the side stream: a launch outside the acut pipeline reuses the first set of partials
    // and folds / moves the rows, so it waits for that cut
    BPR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_keys, 0));
    c->acut_pending = false;
  }
  const bool hot = a.hot_slot != nullptr;
  const bool part = a.snap_meta != nullptr;               // a partial snapshot in front
  const bool acut_fold = acut && c->tune_acut_fold != 0;  // r6: the asynchronous cut with the fold kept on this stream

  // ---- plan
  StreamShape s = {};
  s.n = a.n; s.I = c->I; s.d = c->d; s.G = c->G; s.E = c->E;
  s.sampler = sampler; s.cap_groups = cap_groups; s.run_len = a.run_len; s.force_seen = c->tune_seen;
  s.cus = stream_cus(c); s.grid_cap = stream_grid_cap();
  s.hot = hot; s.hot_H = c->hot_H;
  s.tune_hot_lds = c->tune_hot_lds; s.tune_hot_lds_force = c->tune_hot_lds_force != 0;
  s.tune_lds_block = c->tune_lds_block; s.tune_lds_tail = c->tune_lds_tail;
  // The LDS-tier kernel has FULL instantiations only, reads a snapshot sorted whole, and reads a hot row as Q + its
  // own LDS delta — which leaves out what the global block holds.  So: not in r4's asynchronous-cut pipeline (the
  // deltas stay in the block from launch to launch), nor under the hot tier while the block still holds an earlier
  // launch's deltas that no bpr_hot_exchange with cut = 1 / bpr_sync_cut has taken out yet (c->hot_uncut).
  s.lds_allowed = c->hot_code != nullptr && c->d == c->G * c->E && !part && (!acut || acut_fold) &&
                  !c->hot_unfolded && !c->hot_uncut;
  StreamPlan p = plan_stream_block(s);
  int occ = 0;
  if (int rc = stream_occupancy(c, sampler, p, &occ)) return rc;
  p = plan_stream(s, p, occ);
  const bool lds = p.kernel == STREAM_LDS;
  a.run_len = p.run_len; a.bm_words = p.bm_words; a.gpw_active = p.gpw_active;
  if (lds) {
    a.lds_L = p.L; a.tail1 = p.tail1; a.tail2 = p.tail2;
    a.hot_slot = c->hot_code;
    a.hot_by_rank = c->hot_by_rank;
    a.lds_only = c->hot_tier ? 0 : 1;
  }
  c->last_run_len = p.run_len;
  c->last_lds_rows = p.L;
  StreamKernelFn kernel = nullptr;
  if (!lds)
    if (int rc = stream_kernel(c, sampler, p.seen, part, &kernel)) return rc;

  // ---- events, the partials' parity, the wide bias
  if (cut || acut)
    if (int rc = ensure_cut_events(c)) return rc;
  if (acut) {
    if (c->ev_launch == nullptr) BPR_HIP_CHECK(hipEventCreateWithFlags(&c->ev_launch, hipEventDisableTiming));
    if (c->side == nullptr) {
      BPR_HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
      c->side_owned = true;
    }
    if (!acut_fold) {
      // the launch after next reuses this launch's partials: two sets, used alternately
      if (a.partials != nullptr) a.partials = c->dev_scalars + (size_t)c->acut_parity * 4 * (STREAM_MAX_GRID + 1);
      c->acut_parity ^= 1;
    }
  }
  if (a.bias != nullptr) {  // the launch works on the bias with one item per line (bpr_kernels.h)
    if (c->bias_w_rows != c->I) {
      hipFree(c->bias_w);
      c->bias_w = nullptr;
      c->bias_w_rows = 0;
      BPR_HIP_CHECK(hipMalloc(&c->bias_w, sizeof(float) * (size_t)c->I * BIAS_LINE));
      c->bias_w_rows = c->I;
    }
    // (re)fill the wide table — unless it is known to equal the dense vector still: the epilogue of
    // the previous launch wrote it back, and nobody has touched the vector since (every entry point
    // of the library that writes it says so; writes of the caller's own: bpr_bias_written)
    if (!(c->bias_track && c->bias_w_valid && c->bias_w_of == c->bias))
      hipLaunchKernelGGL(k_bias_widen, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream, c->bias,
                         c->bias_w, (int32_t)c->I);
    c->bias_w_valid = false;
    c->bias_w_of = c->bias;
    a.bias = c->bias_w;
  }
  // hot tier + cut: fold, reconciliation passes and snapshot cut are ONE pass, bpr_sync_cut, which the
  // caller issues next; the launch leaves it its loss partials too
  const bool defer = cut && hot && c->hot_tier;
  // the write-back rides on the launch's own epilogue where there is one on this stream
  const bool bias_in_epilogue = a.bias != nullptr && (!acut || acut_fold) && !defer;

  // ---- launch
  {
    Timer tm(c, true);
    (void)tm;
    hipEvent_t stop = (acut && !acut_fold) ? c->ev_launch : nullptr;
    if (lds) {
      if (int rc = launch_stream_lds(c, a, sampler, p, stop)) return rc;
    } else {
      hipExtLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.shmem, c->stream, nullptr, stop, 0, a);
    }
  }
  if (hot && c->hot_tier) c->hot_uncut = true;  // this launch's deltas stay in the block for bpr_hot_exchange
  if (a.bias != nullptr && !bias_in_epilogue)
    hipLaunchKernelGGL(k_bias_narrow, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream,
                       c->bias_w, c->bias, (int32_t)c->I);
  if (a.bias != nullptr) c->bias_w_valid = true;  // dense == wide again once the write-back has run

  // ---- epilogue
  const bool fold = hot && !c->hot_tier;  // hot tier: the deltas stay for bpr_hot_exchange
  if (acut) {
    // the cut of the next snapshot on the SIDE stream, behind this launch and beside the next one.
    // r6 (acut_fold): the launch stream keeps only what the NEXT launch needs — the fold of the hot block (+ loss
    // statistics, + the item_bias write-back): k_stream_epilogue, a few microseconds — and the 2 x I x d x 4-byte
    // transpose that only the sorter reads goes to the side stream, behind this epilogue (it reads Q while the next
    // launch updates it: a snapshot cut during the launch instead of before it — a little FRESHER than lag 1, inside
    // the same budget).  The block is folded after every launch, so the LDS-tier kernel stays valid.
    // r4: read-only (keys = Q + hot deltas, nothing folded); the cut also sums the loss partials.
    if (acut_fold)
      if (int rc = stream_epilogue(c, a.partials, (int)p.grid, out_scalars, fold, bias_in_epilogue, c->ev_launch))
        return rc;
    const EpilogueCutArgs ec = acut_fold ? cut_args(c, nullptr, 0, nullptr, false, false, false)
                                         : cut_args(c, a.partials, (int)p.grid, out_scalars, hot, false, false);
    BPR_HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_launch, 0));
    hipExtLaunchKernelGGL(k_stream_epilogue_cut, cut_grid(c), dim3(256), 0, c->side, nullptr, c->ev_keys, 0, ec);
    BPR_HIP_CHECK(hipGetLastError());
    mark_keys_cut(c, true, true);
    if (!acut_fold) c->hot_unfolded = hot;
    return BPR_OK;
  }
  if (defer) {
    c->defer_blocks = (int)p.grid;
    c->defer_out = out_scalars;
    c->defer_pending = true;
  } else if (cut) {
    // the epilogue also cuts the next snapshot's keys (k_stream_epilogue_cut) — into the key
    // buffer the split refresh that may still be sorting does NOT read (bpr_ctx.h keysT_buf)
    const EpilogueCutArgs ec = cut_args(c, a.partials, (int)p.grid, out_scalars, hot, true, bias_in_epilogue);
    // the split refresh's side stream waits for this cut: the event rides on the kernel's own
    // completion signal (hipExtLaunchKernelGGL stop event) instead of a marker packet behind it
    static const bool ride = getenv("BPR_CUT_EVENT") == nullptr || atoi(getenv("BPR_CUT_EVENT")) != 0;
    if (ride)
      hipExtLaunchKernelGGL(k_stream_epilogue_cut, cut_grid(c), dim3(256), 0, c->stream, nullptr, c->ev_keys, 0, ec);
    else
      hipLaunchKernelGGL(k_stream_epilogue_cut, cut_grid(c), dim3(256), 0, c->stream, ec);
    mark_keys_cut(c, ride, false);
  } else if (out_scalars != nullptr || fold || bias_in_epilogue) {
    return stream_epilogue(c, a.partials, (int)p.grid, out_scalars, fold, bias_in_epilogue, nullptr);
  }
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

float inv_log1mp(float p) { return (float)(1.0 / log1p(-(double)p)); }


int check_triples(const bpr_ctx* c, const char* who, const int32_t* users,
                         const int32_t* pos, int64_t B) {
  if (int rc = check_bound(c, who)) return rc;
  if (B < 0 || (B > 0 && (users == nullptr || pos == nullptr)))
    return fail(BPR_ERR_INVALID, std::string(who) + ": bad argument");
  return BPR_OK;
}

int refuse_scored(const std::string& who, int32_t sampler) {
  if (!sampler_scored(sampler)) return BPR_OK;
  return fail(BPR_ERR_UNSUPPORTED, who + (sampler == BPR_NEG_WARP ? ": the WARP objective is" : ": dynamic negatives are") +
                                       " fused into the plain-SGD STREAM kernel only (bpr_train_stream)");
}

int check_sampler(const bpr_ctx* c, const char* who, int32_t sampler, float adaptive_p,
                         const int32_t* neg, int64_t B) {
  if (sampler == BPR_NEG_GIVEN) {
    if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, std::string(who) + ": neg is NULL");
    return BPR_OK;
  }
  if (sampler != BPR_NEG_UNIFORM && sampler != BPR_NEG_ADAPTIVE && !sampler_scored(sampler))
    return fail(BPR_ERR_INVALID, std::string(who) + ": unknown sampler");
  if (c->indptr == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": seen CSR not bound");
  if (sampler == BPR_NEG_ADAPTIVE) {
    if (!c->have_snapshot)
      return fail(BPR_ERR_INVALID, std::string(who) + ": call bpr_adaptive_refresh first");
    if (!(adaptive_p > 0.f && adaptive_p < 1.f))
      return fail(BPR_ERR_INVALID, std::string(who) + ": adaptive_p not in (0,1)");
  }
  return BPR_OK;
}

// STRICT lazy replay: bring every row to step c->step (rows tracked by lastP / lastQ)
int strict_flush_impl(bpr_ctx* c) {
  // SGD and Adagrad: a dense zero-gradient step moves nothing — no kernel
  if (!opt_kind_lazy(c->opt_kind) || c->GP == nullptr || c->step == 0) return BPR_OK;
  c->bias_w_valid = false;
  if (int rc = check_opt_state(c, "bpr_flush_lazy")) return rc;
  // (accumulated gradients of a batch in flight are left alone: the flush only advances w / m / v
  // and the rows' last-step marks, bpr_apply then finds nothing left to replay)
  ApplyArgs a = apply_args(c, c->step);
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_flush_lazy<T::G, T::E>), dim3(grid_for(c->U, T::G, 0)), dim3(256), 0,
                       c->stream, a, 0);
    hipLaunchKernelGGL((k_flush_lazy<T::G, T::E>), dim3(grid_for(c->I, T::G, 0)), dim3(256), 0,
                       c->stream, a, 1);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

}  // namespace bpr

using namespace bpr;

extern "C" {

int bpr_version(void) { return BPRCORE_VERSION; }
const char* bpr_last_error(void) { return g_last_error.c_str(); }

int bpr_ctx_create(bpr_ctx** out, int device_id, void* hip_stream) {
  if (out == nullptr) return fail(BPR_ERR_INVALID, "bpr_ctx_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(BPR_ERR_HIP, "bpr_ctx_create: no HIP device visible (libbprcore has no CPU path)");
  if (device_id < 0 || device_id >= ndev)
    return fail(BPR_ERR_INVALID, "bpr_ctx_create: bad device id");
  BPR_HIP_CHECK(hipSetDevice(device_id));
  bpr_ctx* c = new (std::nothrow) bpr_ctx();
  if (c == nullptr) return fail(BPR_ERR_NOMEM, "bpr_ctx_create: out of host memory");
  c->device = device_id;
  c->stream = (hipStream_t)hip_stream;
  if (hipMalloc(&c->dev_scalars, sizeof(float) * 2 * 4 * (size_t)(STREAM_MAX_GRID + 1)) != hipSuccess) {
    delete c;
    return fail(BPR_ERR_HIP, "bpr_ctx_create: hipMalloc failed");
  }
  *out = c;
  return BPR_OK;
}

int bpr_ctx_destroy(bpr_ctx* c) {
  if (c == nullptr) return BPR_OK;
  hipSetDevice(c->device);
  // The caller's streams may be GONE by now: a garbage collector destroys the objects of a finished
  // trainer in any order, and hipStreamSynchronize on a destroyed (CU-masked) stream aborts inside the
  // runtime ("std::system_error: Invalid argument") or hangs — the intermittent failure of the two-rank
  // parity run (r5).  So: wait for the DEVICE, and do whatever cleanup work is left on the default stream.
  hipDeviceSynchronize();
  c->stream = nullptr;
  if (!c->side_owned) c->side = nullptr;
  free_strict_scratch(c);
  comm_free(c, false);  // (no fold into tables that may be gone)
  refresh_free(c);
  side_free(c);
  vs_free(c);
  hipFree(c->bias_w);
  hipFree(c->dev_scalars);
  if (c->ev_launch) hipEventDestroy(c->ev_launch);
  for (auto e : c->ev_start) hipEventDestroy(e);
  for (auto e : c->ev_stop) hipEventDestroy(e);
  delete c;
  return BPR_OK;
}

int bpr_set_stream(bpr_ctx* c, void* hip_stream) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_stream: ctx is NULL");
  c->stream = (hipStream_t)hip_stream;
  return BPR_OK;
}

int bpr_bind_tables(bpr_ctx* c, float* P, int64_t U, float* Q, int64_t I, int32_t d,
                    float* item_bias, int32_t pad_user, int32_t pad_item) {
  if (c == nullptr || P == nullptr || Q == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: NULL argument");
  if (U < 1 || I < 2 || U >= ((int64_t)1 << 30) || I >= ((int64_t)1 << 30))
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: table sizes out of range");
  if (d < 1 || d > 1024)
    return fail(BPR_ERR_UNSUPPORTED, "bpr_bind_tables: embedding dim must be in [1, 1024]");
  if (((uintptr_t)P | (uintptr_t)Q) & 3u)
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: tables must be 4-byte aligned");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->U != U || c->I != I || c->d != d) {
    BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
    free_strict_scratch(c);
    refresh_free(c);
    vs_free(c);
  } else if (c->vs_active && (c->P != P || c->Q != Q || c->bias != item_bias)) {
    if (int rc = vs_leave(c)) return rc;  // pending steps belong to the tables bound so far
  }
  c->P = P; c->Q = Q; c->bias = item_bias;
  c->bias_w_valid = false;
  c->keys_cut = false;
  c->U = U; c->I = I; c->d = d;
  c->pad_user = pad_user; c->pad_item = pad_item;
  const GroupShape g = group_shape(d);  // (bpr_group_shape.h: G = 32 up to d = 128, else 64)
  c->G = g.G;
  c->E = g.E;
  return BPR_OK;
}

int bpr_bind_seen_csr(bpr_ctx* c, const int64_t* indptr, const int32_t* indices) {
  if (c == nullptr || indptr == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_bind_seen_csr: NULL argument");
  c->indptr = indptr;
  c->indices = indices;
  c->heavy_for = nullptr;  // the heavy users' bitmaps belong to the CSR bound before: rebuilt lazily
  return BPR_OK;
}

int bpr_bind_item_weights(bpr_ctx* c, const float* accept, const int32_t* alias) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bind_item_weights: ctx is NULL");
  if ((accept == nullptr) != (alias == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_bind_item_weights: accept and alias go together");
  c->w_accept = accept;
  c->w_alias = alias;
  return BPR_OK;
}

int bpr_set_reg(bpr_ctx* c, float alpha_user, float alpha_item, float alpha_neg) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_reg: ctx is NULL");
  c->au = alpha_user; c->ai = alpha_item; c->an = alpha_neg;
  return BPR_OK;
}

int bpr_set_optimizer(bpr_ctx* c, int32_t kind, const bpr_opt_params* params) {
  // the kind and its hyper-parameters first (bpr_opt_plan.h): a refusal of those needs no ctx
  if (const char* msg = opt_params_error(kind, params)) return fail(BPR_ERR_INVALID, msg);
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_optimizer: ctx is NULL");
  if (c->vs_active && (kind != c->opt_kind || memcmp(&c->opt, params, sizeof(*params)) != 0)) {
    // batched STREAM: pending steps and the replay of missed ones use the hyper-parameters in
    // force when they were taken — bring every row to "now" before those change
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;
  }
  c->opt_kind = kind;
  c->opt = *params;
  return BPR_OK;
}

int bpr_bind_opt_state(bpr_ctx* c, float* m_P, float* v_P, float* m_Q, float* v_Q, float* m_bias,
                       float* v_bias) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bind_opt_state: ctx is NULL");
  if (c->vs_active && (c->mP != m_P || c->vP != v_P || c->mQ != m_Q || c->vQ != v_Q ||
                       c->mb != m_bias || c->vb != v_bias)) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;  // finish with the state tensors bound so far
  }
  c->mP = m_P; c->vP = v_P; c->mQ = m_Q; c->vQ = v_Q; c->mb = m_bias; c->vb = v_bias;
  return BPR_OK;
}

// ---- sampling -----------------------------------------------------------------------------------
static int launch_sample(bpr_ctx* c, int what, SampleArgs a) {
  if (a.n <= 0) return BPR_OK;
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    const unsigned grid = grid_for(a.n, G, 0);
    // adaptive picks walk hundreds of candidates: an LDS seen-bitmap per group when the block's
    // bitmaps fit 64 KiB; the uniform sampler tests a handful and searches the CSR directly
    const int words = (int)(((c->I + 31) / 32 + 3) / 4 * 4);
    const size_t lds = (size_t)(256 / G) * words * sizeof(uint32_t);
    const bool no_bm = c->tune_seen == 1;
    // (one block per CU is plenty for a single batch, so the bitmaps may take most of the 160 KB)
    constexpr size_t SAMPLE_LDS_MAX = 144 * 1024;
    const bool bm = what != SAMPLE_UNIFORM && lds <= SAMPLE_LDS_MAX && !no_bm;
    a.bm_words = bm ? words : 0;
    if (bm && lds > 64 * 1024) {
      static bool raised = false;  // per (G, E) instantiation of this lambda
      if (!raised) {
        BPR_HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_sample<G, E, SAMPLE_ADAPTIVE, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)SAMPLE_LDS_MAX));
        BPR_HIP_CHECK(hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_sample<G, E, SAMPLE_PICK, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)SAMPLE_LDS_MAX));
        raised = true;
      }
    }
    if (what == SAMPLE_UNIFORM)
      hipLaunchKernelGGL((k_sample<G, E, SAMPLE_UNIFORM, false>), dim3(grid), dim3(256), 0,
                         c->stream, a);
    else if (what == SAMPLE_ADAPTIVE && bm)
      hipLaunchKernelGGL((k_sample<G, E, SAMPLE_ADAPTIVE, true>), dim3(grid), dim3(256), lds,
                         c->stream, a);
    else if (what == SAMPLE_ADAPTIVE)
      hipLaunchKernelGGL((k_sample<G, E, SAMPLE_ADAPTIVE, false>), dim3(grid), dim3(256), 0,
                         c->stream, a);
    else if (bm)
      hipLaunchKernelGGL((k_sample<G, E, SAMPLE_PICK, true>), dim3(grid), dim3(256), lds, c->stream,
                         a);
    else
      hipLaunchKernelGGL((k_sample<G, E, SAMPLE_PICK, false>), dim3(grid), dim3(256), 0, c->stream,
                         a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

static SampleArgs sample_args(const bpr_ctx* c) {
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  (void)snapshot_complete_impl(const_cast<bpr_ctx*>(c));  // the sampler kernels read a snapshot sorted whole
  a.P = c->P; a.I = c->I; a.d = c->d;
  a.indptr = c->indptr; a.indices = c->indices;
  a.order = c->order; a.sigma = c->sigma;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  a.mP = c->mP; a.vP = c->vP; a.lastP = opt_kind_lazy(c->opt_kind) ? c->lastP : nullptr;
  a.o = opt_dev(c, c->step + 1);
  return a;
}

int bpr_sample_uniform(bpr_ctx* c, const int32_t* users, int64_t B, uint64_t seed, uint64_t offset,
                       int32_t* neg_out) {
  if (int rc = check_bound(c, "bpr_sample_uniform")) return rc;
  if (c->indptr == nullptr) return fail(BPR_ERR_INVALID, "bpr_sample_uniform: seen CSR not bound");
  if (users == nullptr || neg_out == nullptr || B < 0)
    return fail(BPR_ERR_INVALID, "bpr_sample_uniform: bad argument");
  SampleArgs a = sample_args(c);
  a.users = users; a.n = B; a.seed = seed; a.offset = offset; a.neg = neg_out;
  return launch_sample(c, SAMPLE_UNIFORM, a);
}

int bpr_adaptive_refresh(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh")) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active)  // batched STREAM: the snapshot must see the item rows as of "now"
    if (int rc = vs_flush(c, false, true)) return rc;
  const int world = comm_world(c);
  if (world > 1 && c->d % world == 0 && !c->refresh_pending) {
    // several ranks behind one communicator: every rank sorts its share of the factors of its own
    // replica, an all-gather hands everybody every factor's order, the same snapshot is published
    const int per = c->d / world, r = comm_rank(c);
    if (int rc = refresh_impl(c, false, r * per, (r + 1) * per)) return rc;
    const int back = c->have_snapshot ? (c->snap_front ^ 1) : c->snap_front;
    if (int rc = comm_gather_snapshot(c, c->order_alloc[back] + BPR_ORDER_PAD, c->sigma_buf[back], per))
      return rc;
    return refresh_publish_impl(c);
  }
  return refresh_impl(c, false, 0, c->d);
}

int bpr_adaptive_refresh_begin(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh_begin", c == nullptr || !c->keys_cut)) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active)
    if (int rc = vs_flush(c, false, true)) return rc;
  return refresh_impl(c, true, 0, c->d);
}

int bpr_adaptive_refresh_commit(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh_commit", false)) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  return refresh_commit_impl(c);
}

int bpr_adaptive_refresh_part(bpr_ctx* c, int32_t f_lo, int32_t f_hi) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh_part")) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active)
    if (int rc = vs_flush(c, false, true)) return rc;
  return refresh_impl(c, false, f_lo, f_hi);
}

int bpr_adaptive_refresh_publish(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh_publish")) return rc;
  return refresh_publish_impl(c);
}

int bpr_adaptive_snapshot_ptrs(bpr_ctx* c, int32_t back, void** order_host, void** sigma_host) {
  if (int rc = check_bound(c, "bpr_adaptive_snapshot_ptrs")) return rc;
  if (order_host == nullptr || sigma_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_adaptive_snapshot_ptrs: NULL argument");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = refresh_alloc(c)) return rc;
  if (!back)
    if (int rc = snapshot_complete_impl(c)) return rc;
  const int front = c->snap_front;
  const int which = back ? (c->have_snapshot ? front ^ 1 : front) : front;
  *order_host = (void*)(c->order_alloc[which] + BPR_ORDER_PAD);
  *sigma_host = (void*)c->sigma_buf[which];
  return BPR_OK;
}

int bpr_adaptive_snapshot_partial(bpr_ctx* c, int32_t* partial_host) {
  if (c == nullptr || partial_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_adaptive_snapshot_partial: NULL argument");
  *partial_host = (c->have_snapshot && c->meta_front != nullptr) ? 1 : 0;
  return BPR_OK;
}

int bpr_adaptive_refresh_info(bpr_ctx* c, int32_t* info_host) {
  if (int rc = check_bound(c, "bpr_adaptive_refresh_info")) return rc;
  if (info_host == nullptr) return fail(BPR_ERR_INVALID, "bpr_adaptive_refresh_info: info_host is NULL");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  return refresh_info_impl(c, info_host);
}

int bpr_adaptive_refresh_pending(bpr_ctx* c, int32_t* pending_host) {
  if (c == nullptr || pending_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_adaptive_refresh_pending: NULL argument");
  *pending_host = c->refresh_pending ? 1 : 0;
  return BPR_OK;
}

int bpr_set_side_stream(bpr_ctx* c, void* hip_stream) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_side_stream: ctx is NULL");
  if (c->refresh_pending)
    return fail(BPR_ERR_INVALID, "bpr_set_side_stream: a split refresh is pending");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->side != nullptr) {
    BPR_HIP_CHECK(hipStreamSynchronize(c->side));
    if (c->side_owned) hipStreamDestroy(c->side);
  }
  c->side = (hipStream_t)hip_stream;
  c->side_owned = false;
  return BPR_OK;
}

int bpr_stream_create(int device_id, const uint32_t* cu_mask, int32_t mask_words, void** stream_out) {
  if (stream_out == nullptr || mask_words < 0 || (mask_words > 0 && cu_mask == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_stream_create: bad argument");
  BPR_HIP_CHECK(hipSetDevice(device_id));
  hipStream_t st = nullptr;
  if (mask_words == 0)
    BPR_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  else
    BPR_HIP_CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask_words, cu_mask));
  *stream_out = (void*)st;
  return BPR_OK;
}

int bpr_stream_destroy(void* hip_stream) {
  if (hip_stream == nullptr) return BPR_OK;
  BPR_HIP_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
  BPR_HIP_CHECK(hipStreamDestroy((hipStream_t)hip_stream));
  return BPR_OK;
}

int bpr_sample_adaptive(bpr_ctx* c, const int32_t* users, int64_t B, float p, uint64_t seed,
                        uint64_t offset, int32_t* neg_out, int32_t* factor_out,
                        int32_t* rank_out) {
  if (int rc = check_bound(c, "bpr_sample_adaptive")) return rc;
  if (c->indptr == nullptr) return fail(BPR_ERR_INVALID, "bpr_sample_adaptive: seen CSR not bound");
  if (!c->have_snapshot)
    return fail(BPR_ERR_INVALID, "bpr_sample_adaptive: call bpr_adaptive_refresh first");
  if (!(p > 0.f && p < 1.f)) return fail(BPR_ERR_INVALID, "bpr_sample_adaptive: p not in (0,1)");
  if (users == nullptr || neg_out == nullptr || B < 0)
    return fail(BPR_ERR_INVALID, "bpr_sample_adaptive: bad argument");
  if (int rc = vs_leave(c)) return rc;  // reads the live user rows
  if (int rc = snapshot_complete_impl(c)) return rc;  // (sample_args cannot report it)
  SampleArgs a = sample_args(c);
  a.users = users; a.n = B; a.seed = seed; a.offset = offset;
  a.neg = neg_out; a.factor_out = factor_out; a.rank_out = rank_out;
  a.inv_log1mp = inv_log1mp(p);
  return launch_sample(c, SAMPLE_ADAPTIVE, a);
}

int bpr_adaptive_pick(bpr_ctx* c, const int32_t* users, const int32_t* factor, const int32_t* rank,
                      int64_t B, int32_t* neg_out) {
  if (int rc = check_bound(c, "bpr_adaptive_pick")) return rc;
  if (c->indptr == nullptr || !c->have_snapshot)
    return fail(BPR_ERR_INVALID, "bpr_adaptive_pick: seen CSR / snapshot missing");
  if (!users || !factor || !rank || !neg_out || B < 0)
    return fail(BPR_ERR_INVALID, "bpr_adaptive_pick: bad argument");
  if (int rc = snapshot_complete_impl(c)) return rc;  // (sample_args cannot report it)
  SampleArgs a = sample_args(c);
  a.users = users; a.factor_in = factor; a.rank_in = rank; a.n = B; a.neg = neg_out;
  return launch_sample(c, SAMPLE_PICK, a);
}

int bpr_adaptive_get_snapshot(bpr_ctx* c, int32_t* order_out, float* sigma_out) {
  if (int rc = check_bound(c, "bpr_adaptive_get_snapshot")) return rc;
  if (!c->have_snapshot) return fail(BPR_ERR_INVALID, "bpr_adaptive_get_snapshot: no snapshot");
  if (int rc = snapshot_complete_impl(c)) return rc;
  if (order_out)
    BPR_HIP_CHECK(hipMemcpyAsync(order_out, c->order, sizeof(int32_t) * (size_t)c->d * c->I,
                                 hipMemcpyDeviceToDevice, c->stream));
  if (sigma_out)
    BPR_HIP_CHECK(hipMemcpyAsync(sigma_out, c->sigma, sizeof(float) * c->d,
                                 hipMemcpyDeviceToDevice, c->stream));
  return BPR_OK;
}

// ---- hot path -----------------------------------------------------------------------------------
int bpr_forward(bpr_ctx* c, const int32_t* users, const int32_t* pos, const int32_t* neg,
                int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  if (int rc = check_triples(c, "bpr_forward", users, pos, B)) return rc;
  if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, "bpr_forward: neg is NULL");
  if (int rc = vs_leave(c)) return rc;
  TripleArgs a = triple_args(c);
  a.users = users; a.pos = pos; a.neg = neg; a.n = B;
  a.lpos = out_logits_pos; a.lneg = out_logits_neg; a.scalars = out_scalars;
  return launch_triples<MODE_FORWARD>(c, a, false);
}

int bpr_forward_grad(bpr_ctx* c, const int32_t* users, const int32_t* pos, const int32_t* neg,
                     int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars) {
  if (int rc = check_triples(c, "bpr_forward_grad", users, pos, B)) return rc;
  if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, "bpr_forward_grad: neg is NULL");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;
  if (int rc = ensure_strict_scratch(c)) return rc;
  TripleArgs a = triple_args(c);
  a.users = users; a.pos = pos; a.neg = neg; a.n = B;
  a.lpos = out_logits_pos; a.lneg = out_logits_neg; a.scalars = out_scalars;
  c->pending += 3 * B;
  if (c->pending > c->U + c->I) c->pending = c->U + c->I;
  return launch_triples<MODE_GRAD>(c, a, true);
}

int bpr_apply(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_apply")) return rc;
  c->keys_cut = false;
  c->bias_w_valid = false;  // writes the item_bias
  if (int rc = check_opt_state(c, "bpr_apply")) return rc;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = ensure_strict_scratch(c)) return rc;
  c->step += 1;
  if (c->pending > 0) {
    ApplyArgs a = apply_args(c, c->step);
    int rc = dispatch_ge(c->G, c->E, [&](auto tag) -> int {
      using T = decltype(tag);
      const unsigned grid = (unsigned)((c->pending * T::G + 255) / 256);
      hipLaunchKernelGGL((k_apply<T::G, T::E>), dim3(grid), dim3(256), 0, c->stream, a);
      BPR_HIP_CHECK(hipGetLastError());
      return BPR_OK;
    });
    if (rc) return rc;
    c->cnt_sel ^= 1;  // the kernel cleared the other counter
    c->pending = 0;
  }
  return BPR_OK;
}

int bpr_discard_grad(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_discard_grad")) return rc;
  if (c->GP == nullptr || c->pending == 0) return BPR_OK;
  ApplyArgs a = apply_args(c, c->step);
  int rc = dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    const unsigned grid = (unsigned)((c->pending * T::G + 255) / 256);
    hipLaunchKernelGGL((k_discard<T::G, T::E>), dim3(grid), dim3(256), 0, c->stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
  if (rc) return rc;
  c->cnt_sel ^= 1;  // the kernel cleared the other counter
  c->pending = 0;
  return BPR_OK;
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

static int train_stream_impl(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg,
                             int64_t n, int32_t sampler, float adaptive_p, uint64_t seed,
                             uint64_t offset, int64_t max_inflight, float* out_scalars, bool cut,
                             bool acut = false) {
  if (acut)  // (no snapshot to cut)
    if (int rc = refuse_scored("bpr_train_stream_acut", sampler)) return rc;
  if (c != nullptr) c->acut_call = acut;  // (check_bound folds pending hot deltas for everybody else)
  const int rc0 = check_triples(c, "bpr_train_stream", users, pos, n);
  if (c != nullptr) c->acut_call = false;
  if (rc0) return rc0;
  c->keys_cut = false;  // the item table moves
  if (int rc = check_sampler(c, "bpr_train_stream", sampler, adaptive_p, neg, n)) return rc;
  if (c->opt_kind != BPR_OPT_SGD)
    return fail(BPR_ERR_UNSUPPORTED,
                "bpr_train_stream: this launch implements plain SGD only; momentum / Adam / RMSprop / "
                "Adagrad run through bpr_train_stream_batched (one launch per refresh period) or STRICT "
                "(bpr_forward_grad + bpr_apply)");
  if (c->pending != 0)
    return fail(BPR_ERR_INVALID, "bpr_train_stream: unapplied STRICT gradients pending");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = vs_leave(c)) return rc;
  if (n >= ((int64_t)1 << 31) || c->U * c->d >= ((int64_t)1 << 31) ||
      c->I * c->d >= ((int64_t)1 << 31))
    return fail(BPR_ERR_UNSUPPORTED,
                "bpr_train_stream: n and rows*d must be < 2^31 (32-bit offsets in the kernel)");
  StreamArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P; a.Q = c->Q; a.bias = c->bias;
  a.indptr = c->indptr; a.indices = c->indices;
  a.order = c->order; a.sigma = c->sigma;
  if (c->meta_front != nullptr && c->keys_front_stale)
    return fail(BPR_ERR_INVALID, "bpr_train_stream: the partial snapshot in front was sorted from keys a later cut has "
                                 "overwritten; commit the pending refresh first");
  a.snap_meta = c->meta_front;
  a.snap_keys = c->meta_front != nullptr ? c->keys_front : nullptr;
  a.users = users; a.pos = pos; a.neg = neg;
  a.partials = out_scalars != nullptr ? c->dev_scalars : nullptr;
  a.seed = seed; a.offset = offset;
  a.n = (int32_t)n; a.I = (int32_t)c->I; a.d = c->d;
  a.pad_user = c->pad_user; a.pad_item = c->pad_item;
  a.run_len = c->run_len;  // 0: launch_stream picks it from the launch size and the chip's occupancy
  a.grouped = c->grouped;
  a.au = c->au; a.ai = c->ai; a.an = c->an; a.lr = c->opt.lr;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  a.inv_log1mp = sampler == BPR_NEG_ADAPTIVE ? inv_log1mp(adaptive_p) : 0.f;
  a.dyn_M = c->dyn_M;
  a.warp_N = c->warp_N;
  a.warp_margin = c->warp_margin;
  if (sampler != BPR_NEG_GIVEN) {
    if (int rc = heavy_build_impl(c)) return rc;
    a.heavy_off = c->heavy_off;
    a.heavy_bits = c->heavy_bits;
    a.heavy_T = c->heavy_T;
  }
  if (c->hot_H > 0) {
    a.hot_slot = c->hot_slot;
    a.hot_delta = c->hot_delta;
    a.hot_H = c->hot_H;
    a.hot_rmask = c->hot_R - 1;
  }
  if (acut && (c->hot_tier || c->vs_active))
    return fail(BPR_ERR_INVALID, "bpr_train_stream_acut: not under the hot tier / batched STREAM bookkeeping");
  if (acut)
    if (int rc = refresh_alloc(c)) return rc;
  return launch_stream(c, a, sampler, max_inflight, out_scalars, cut && !acut, acut);
}

int bpr_train_stream(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg, int64_t n,
                     int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
                     int64_t max_inflight, float* out_scalars) {
  return train_stream_impl(c, users, pos, neg, n, sampler, adaptive_p, seed, offset, max_inflight,
                           out_scalars, false);
}

int bpr_train_stream_cut(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg,
                         int64_t n, int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
                         int64_t max_inflight, float* out_scalars) {
  if (n <= 0)
    return fail(BPR_ERR_INVALID, "bpr_train_stream_cut: needs a non-empty launch (the cut rides "
                                 "on its epilogue)");
  return train_stream_impl(c, users, pos, neg, n, sampler, adaptive_p, seed, offset, max_inflight,
                           out_scalars, true);
}

int bpr_train_stream_acut(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg,
                          int64_t n, int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
                          int64_t max_inflight, float* out_scalars) {
  if (n <= 0)
    return fail(BPR_ERR_INVALID, "bpr_train_stream_acut: needs a non-empty launch");
  return train_stream_impl(c, users, pos, neg, n, sampler, adaptive_p, seed, offset, max_inflight,
                           out_scalars, true, true);
}

int bpr_hot_fold(bpr_ctx* c) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_hot_fold: ctx is NULL");
  return hot_fold_impl(c);
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
  if (defer) {
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->dev_scalars,
                       (int)stat_blocks, out_scalars);
    BPR_HIP_CHECK(hipGetLastError());
  }
  return BPR_OK;
}

int bpr_item_delta(const float* q, const float* base, float* own, float* tot, int64_t n,
                   void* hip_stream) {
  if (n < 0 || (n > 0 && (!q || !base || !own || !tot)))
    return fail(BPR_ERR_INVALID, "bpr_item_delta: bad argument");
  if (n == 0) return BPR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 1023) / 1024, 4096);
  hipLaunchKernelGGL(k_item_delta, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, q, base, own,
                     tot, n);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

int bpr_item_fold(float* q, float* base, const float* own, const float* tot, float scale,
                  int32_t rebase, int64_t n, void* hip_stream) {
  if (n < 0 || (n > 0 && (!q || !base || !own || !tot)))
    return fail(BPR_ERR_INVALID, "bpr_item_fold: bad argument");
  if (n == 0) return BPR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 1023) / 1024, 4096);
  hipLaunchKernelGGL(k_item_fold, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, q, base, own,
                     tot, scale, rebase, n);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

int bpr_item_fold_delta(float* q, float* base, float* own, float* tot, float scale, int64_t n,
                        void* hip_stream) {
  if (n < 0 || (n > 0 && (!q || !base || !own || !tot)))
    return fail(BPR_ERR_INVALID, "bpr_item_fold_delta: bad argument");
  if (n == 0) return BPR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 1023) / 1024, 4096);
  hipLaunchKernelGGL(k_item_fold_delta, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, q, base,
                     own, tot, scale, n);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

int bpr_set_hot_rows(bpr_ctx* c, int32_t hot_rows, int32_t replicas) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_hot_rows: ctx is NULL");
  if (hot_rows < 0 || hot_rows > 32768)
    return fail(BPR_ERR_INVALID, "bpr_set_hot_rows: hot_rows must be in [0, 32768]");
  if (hot_rows > 0 && replicas != 1 && replicas != 2 && replicas != 4 && replicas != 8)
    return fail(BPR_ERR_INVALID, "bpr_set_hot_rows: replicas must be 1, 2, 4 or 8");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
  hot_free(c);  // rebuilt by the next bpr_plan_epoch
  c->hot_rows_opt = hot_rows;
  c->hot_reps_opt = hot_rows > 0 ? replicas : 0;
  return BPR_OK;
}

int bpr_set_hot_lds(bpr_ctx* c, int32_t rows, int32_t always) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_hot_lds: ctx is NULL");
  if (rows < 0 || rows > 32767) return fail(BPR_ERR_INVALID, "bpr_set_hot_lds: rows must be in [0, 32767]");
  c->tune_hot_lds = rows;
  c->tune_hot_lds_force = always != 0;
  return BPR_OK;
}

int bpr_stream_lds_rows(bpr_ctx* c) {
  return c == nullptr ? 0 : c->last_lds_rows;
}

int bpr_set_hot_items(bpr_ctx* c, const int32_t* items_host, int32_t H, const uint32_t* counts_host) {
  if (int rc = check_bound(c, "bpr_set_hot_items")) return rc;
  if (H < 0 || H > 32768 || H >= c->I || (H > 0 && items_host == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_set_hot_items: need 0 <= H <= min(32768, I - 1) item ids");
  if (c->hot_tier) return fail(BPR_ERR_INVALID, "bpr_set_hot_items: the hot tier is on (bpr_hot_tier_end first)");
  std::vector<char> seen((size_t)c->I, 0);
  for (int k = 0; k < H; ++k) {
    const int32_t it = items_host[k];
    if (it < 0 || it >= c->I || it == c->pad_item || seen[it])
      return fail(BPR_ERR_INVALID, "bpr_set_hot_items: ids must be distinct item rows, not the pad row");
    seen[it] = 1;
  }
  BPR_HIP_CHECK(hipSetDevice(c->device));
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return hot_set_items_impl(c, items_host, H, counts_host);
}

int bpr_hot_rows(bpr_ctx* c, int32_t* rows_host) {
  if (c == nullptr || rows_host == nullptr) return fail(BPR_ERR_INVALID, "bpr_hot_rows: NULL argument");
  *rows_host = c->hot_H;
  return BPR_OK;
}

int bpr_hot_tier_begin(bpr_ctx* c, float* hot_base) {
  if (int rc = check_bound(c, "bpr_hot_tier_begin")) return rc;
  if (c->hot_H <= 0 || !c->hot_explicit)
    return fail(BPR_ERR_INVALID, "bpr_hot_tier_begin: no hot set (bpr_set_hot_items first: the ranks "
                                 "must agree on it)");
  if (hot_base == nullptr) return fail(BPR_ERR_INVALID, "bpr_hot_tier_begin: hot_base is NULL");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  const int64_t n = (int64_t)c->hot_H * c->d;
  hipLaunchKernelGGL(k_hot_gather, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256),
                     0, c->stream, c->Q, c->hot_items, c->hot_canon, hot_base, c->hot_H, c->d);
  BPR_HIP_CHECK(hipGetLastError());
  c->hot_tier = true;
  return BPR_OK;
}

int bpr_hot_tier_end(bpr_ctx* c) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_hot_tier_end: ctx is NULL");
  if (int rc = flush_deferred_stats(c)) return rc;
  c->hot_tier = false;  // (the caller has folded everything: bpr_hot_exchange with cut = 1 last)
  return BPR_OK;
}

int bpr_hot_exchange(bpr_ctx* c, float* hot_base, float* tot, int32_t fold_prev, int32_t cut,
                     float* cold_base) {
  if (int rc = check_bound(c, "bpr_hot_exchange")) return rc;
  if (!c->hot_tier) return fail(BPR_ERR_INVALID, "bpr_hot_exchange: the hot tier is off (bpr_hot_tier_begin)");
  if (hot_base == nullptr || tot == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_hot_exchange: NULL buffer");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = flush_deferred_stats(c)) return rc;  // a cut launch that was not followed by bpr_sync_cut
  c->keys_cut = false;  // the item table moves
  HotStepArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = c->Q; a.delta = c->hot_delta; a.hot_items = c->hot_items; a.canon = c->hot_canon;
  a.hb = hot_base; a.tot = tot; a.cold_base = cold_base;
  a.H = c->hot_H; a.R = c->hot_R; a.d = c->d; a.fold_prev = fold_prev != 0; a.cut = cut != 0;
  const int64_t n = (int64_t)c->hot_H * c->d;
  hipLaunchKernelGGL(k_hot_step, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0,
                     c->stream, a);
  BPR_HIP_CHECK(hipGetLastError());
  if (cut) c->hot_uncut = false;  // the block is zero again: the next launch may take the LDS tier
  return BPR_OK;
}

int bpr_set_heavy_users(bpr_ctx* c, int32_t threshold, int64_t max_bytes) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_heavy_users: ctx is NULL");
  if (threshold < -1 || max_bytes < 0)
    return fail(BPR_ERR_INVALID, "bpr_set_heavy_users: threshold >= -1, max_bytes >= 0");
  c->heavy_T_opt = threshold;
  if (max_bytes > 0) c->heavy_max_bytes = max_bytes;
  c->heavy_for = nullptr;  // rebuilt by the next sampling STREAM launch
  return BPR_OK;
}

int bpr_heavy_users(bpr_ctx* c, int64_t* n, int32_t* threshold) {
  if (c == nullptr || n == nullptr || threshold == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_heavy_users: NULL argument");
  const bool built = c->heavy_for != nullptr && c->heavy_for == c->indptr;
  *n = built ? c->heavy_n : 0;
  *threshold = built ? c->heavy_T : c->heavy_T_opt;
  return BPR_OK;
}

int bpr_sync_cut(bpr_ctx* c, float* hot_base, float* hot_tot, int32_t hot_fold_prev, float* cold_base,
                 float* cold_own, float* cold_tot, float scale, int32_t cold_mode) {
  if (int rc = check_bound(c, "bpr_sync_cut")) return rc;
  if (cold_mode < 0 || cold_mode > 2 || (cold_mode != 0 && (!cold_base || !cold_own || !cold_tot)))
    return fail(BPR_ERR_INVALID, "bpr_sync_cut: cold_mode 0 | 1 | 2 with base / own / tot");
  if (c->hot_tier && (hot_base == nullptr || hot_tot == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_sync_cut: the hot tier is on: hot_base / hot_tot needed");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = refresh_alloc(c)) return rc;
  if (int rc = ensure_cut_events(c)) return rc;
  SyncCutArgs a;
  memset(&a, 0, sizeof(a));
  a.e = cut_args(c, c->dev_scalars, c->defer_pending ? c->defer_blocks : 0, c->defer_pending ? c->defer_out : nullptr,
                 c->hot_H > 0, false, false);
  a.canon = c->hot_canon; a.hb = hot_base; a.htot = hot_tot;
  a.base = cold_base; a.own = cold_own; a.tot = cold_tot; a.scale = scale;
  a.hot_tier = c->hot_tier ? 1 : 0; a.hot_fold_prev = hot_fold_prev != 0; a.cold_mode = cold_mode;
  hipExtLaunchKernelGGL(k_sync_cut, cut_grid(c), dim3(256), 0, c->stream, nullptr, c->ev_keys, 0, a);
  BPR_HIP_CHECK(hipGetLastError());
  c->defer_pending = false;
  c->hot_uncut = false;  // (the hot-tier step cut the block)
  c->keys_cut = true;   // the next bpr_adaptive_refresh_begin only queues the sort
  c->keys_event = true;
  return BPR_OK;
}

int bpr_set_tuning(bpr_ctx* c, const char* key, int32_t value) {
  if (c == nullptr || key == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_tuning: NULL argument");
  const std::string k = key;
  if (k == "seen" && value >= 0 && value <= 3) c->tune_seen = value;
  else if (k == "vs_direct" && value >= -1 && value <= 1) c->tune_vs_direct = value;
  else if (k == "adam_closed" && (value == 0 || value == 1)) c->tune_adam_closed = value;
  else if (k == "partial_snapshot" && (value == 0 || value == 1)) c->tune_partial = value;
  else if (k == "binned_sort" && (value == 0 || value == 1)) c->tune_binned = value;
  else if (k == "binned_split" && value >= 0 && value <= 16) c->tune_binned_split = value;
  else if (k == "partial_target" && value >= 1 && value <= 1024) c->partial_target = value;
  else if (k == "refresh_sub" && (value == 0 || value == 1 || value == 2 || value == 4)) c->tune_refresh_sub = value;
  else if (k == "lds_block" && value >= 0 && value <= 1024 && value % 64 == 0) c->tune_lds_block = value;
  else if (k == "lds_tail" && value >= 0 && value <= 50) c->tune_lds_tail = value;
  else if (k == "plan_input_sorted" && (value == 0 || value == 1)) c->tune_plan_sorted = value;
  else if (k == "acut_fold" && (value == 0 || value == 1)) c->tune_acut_fold = value;
  else return fail(BPR_ERR_INVALID, "bpr_set_tuning: unknown key or value out of range");
  c->stream_occ.clear();
  return BPR_OK;
}

int bpr_set_bias_tracking(bpr_ctx* c, int32_t on) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_bias_tracking: ctx is NULL");
  c->bias_track = on != 0;
  c->bias_w_valid = false;
  return BPR_OK;
}

int bpr_bias_written(bpr_ctx* c) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bias_written: ctx is NULL");
  c->bias_w_valid = false;
  return BPR_OK;
}

int bpr_stream_run_len(bpr_ctx* c) {
  return c == nullptr ? 0 : c->last_run_len;
}

// Test hook, not API (tests/test_stream_plan_cpu.py sets its signature): the launch plan of a shape given as plain
// integers — StreamShape's fields in order — and an occupancy; out = StreamPlan's fields in order.  Needs no GPU.
int bpr_test_stream_plan(const int64_t* in, int32_t occ, int64_t* out) {
  StreamShape s = {};
  s.n = in[0]; s.I = in[1]; s.d = (int)in[2]; s.G = (int)in[3]; s.E = (int)in[4];
  s.sampler = (int)in[5]; s.cap_groups = in[6]; s.run_len = (int)in[7]; s.force_seen = (int)in[8];
  s.cus = (int)in[9]; s.grid_cap = in[10]; s.hot = in[11] != 0; s.hot_H = (int)in[12];
  s.tune_hot_lds = (int)in[13]; s.tune_hot_lds_force = in[14] != 0;
  s.tune_lds_block = (int)in[15]; s.tune_lds_tail = (int)in[16]; s.lds_allowed = in[17] != 0;
  const StreamPlan p = plan_stream(s, plan_stream_block(s), occ);
  const int64_t v[] = {p.kernel, p.seen, p.block, p.grid, (int64_t)p.shmem, p.bm_words, p.gpw_active, p.run_len,
                       p.L, p.tail1, p.tail2};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}

// Test hook, not API (tests/test_refresh_plan_cpu.py sets its signature): the sorter plan of a refresh given as plain
// integers — RefreshShape's fields in order; out = RefreshPlan's fields in order.  Needs no GPU.
int bpr_test_refresh_plan(const int64_t* in, int64_t* out) {
  RefreshShape s = {};
  s.I = in[0]; s.nf = (int)in[1]; s.split = in[2] != 0; s.part = in[3] != 0;
  s.tune_binned = (int)in[4]; s.tune_binned_split = (int)in[5]; s.tune_refresh_sub = (int)in[6];
  s.tune_partial = (int)in[7]; s.no_fast = in[8] != 0;
  const RefreshPlan p = plan_refresh(s);
  const int64_t v[] = {p.route, p.sub, p.len, p.g, p.sitems, p.items, p.fallback, p.fb_items, p.wide, p.partial};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}

int bpr_set_stream_opts(bpr_ctx* c, int32_t grouped_by_user, int32_t run_len) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_stream_opts: ctx is NULL");
  if (run_len < 0 || run_len > 30)
    return fail(BPR_ERR_INVALID, "bpr_set_stream_opts: run_len must be 0 (by launch size) or in [1, 30] (one lane of a "
                                 "32-lane group per triple of the run, plus two neighbours)");
  c->grouped = grouped_by_user != 0;
  c->run_len = run_len;
  return BPR_OK;
}

int bpr_plan_epoch(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n,
                   int64_t chunk, uint64_t seed, int32_t* users_out, int32_t* pos_out) {
  if (int rc = check_bound(c, "bpr_plan_epoch")) return rc;
  if (n < 0 || chunk < 1 || (n > 0 && (!users_in || !pos_in || !users_out || !pos_out)))
    return fail(BPR_ERR_INVALID, "bpr_plan_epoch: bad argument");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  return plan_epoch_impl(c, users_in, pos_in, n, chunk, seed, users_out, pos_out);
}

int bpr_plan_chunk(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n, int64_t chunk,
                   uint64_t seed, int64_t index, int32_t* users_out, int32_t* pos_out, int32_t on_side) {
  if (int rc = check_bound(c, "bpr_plan_chunk")) return rc;
  if (n < 1 || n >= ((int64_t)1 << 31) || chunk < 1 || index < 0 || !users_in || !pos_in || !users_out ||
      !pos_out)
    return fail(BPR_ERR_INVALID, "bpr_plan_chunk: bad argument");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->hot_key_ptr != pos_in || c->hot_key_n != n) {  // new training set: measure popularity (as
    if (int rc = hot_build_impl(c, pos_in, n)) return rc;  // bpr_plan_epoch does)
  }
  if (!on_side) return plan_chunk_impl(c, users_in, pos_in, n, chunk, seed, index, users_out, pos_out, c->stream);
  // behind the split refresh's sort on the side stream; what bpr_adaptive_refresh_commit waits for
  // then covers this chunk too (one event, no extra packet on the launch stream)
  if (c->side == nullptr || !c->refresh_pending)
    return fail(BPR_ERR_INVALID, "bpr_plan_chunk: on_side needs a split refresh in flight "
                                 "(bpr_adaptive_refresh_begin first)");
  if (int rc = plan_chunk_impl(c, users_in, pos_in, n, chunk, seed, index, users_out, pos_out, c->side))
    return rc;
  BPR_HIP_CHECK(hipEventRecord(c->ev_sorted, c->side));
  return BPR_OK;
}

int bpr_flush_lazy(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_flush_lazy")) return rc;
  c->keys_cut = false;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active) return vs_flush(c, true, true);  // batched STREAM bookkeeping is live
  return strict_flush_impl(c);
}

int bpr_flush_items(bpr_ctx* c) {
  if (int rc = check_bound(c, "bpr_flush_items")) return rc;
  c->keys_cut = false;
  c->bias_w_valid = false;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->vs_active) return vs_flush(c, false, true);
  if (!opt_kind_lazy(c->opt_kind) || c->GP == nullptr || c->step == 0) return BPR_OK;
  if (int rc = check_opt_state(c, "bpr_flush_items")) return rc;
  ApplyArgs a = apply_args(c, c->step);
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_flush_lazy<T::G, T::E>), dim3(grid_for(c->I, T::G, 0)), dim3(256), 0,
                       c->stream, a, 1);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

int bpr_get_step_host(bpr_ctx* c, int64_t* step_host) {
  if (c == nullptr || step_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_get_step_host: NULL argument");
  *step_host = c->step;
  return BPR_OK;
}

int bpr_set_step(bpr_ctx* c, int64_t step) {
  if (c == nullptr || step < 0) return fail(BPR_ERR_INVALID, "bpr_set_step: bad argument");
  if (c->vs_active) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;
  }
  // rows are assumed flushed at `step` (a checkpoint is written after bpr_flush_lazy)
  c->step = step;
  if (c->lastP != nullptr) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastP, (int)step, (size_t)c->U, c->stream));
    BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastQ, (int)step, (size_t)c->I, c->stream));
  }
  return BPR_OK;
}

int bpr_set_sampler_iter(bpr_ctx* c, int64_t iteration) {
  if (c == nullptr || iteration < 0)
    return fail(BPR_ERR_INVALID, "bpr_set_sampler_iter: bad argument");
  c->strict_iter = iteration;
  return BPR_OK;
}

int bpr_timing_enable(bpr_ctx* c, int32_t on) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_timing_enable: ctx is NULL");
  if (int rc = drain_timing(c)) return rc;
  c->timing = on != 0;
  c->timing_stride = on > 1 ? on : 1;
  c->timing_seen = 0;
  c->timed_ms = 0.0;
  c->timed_launches = 0;
  return BPR_OK;
}

int bpr_timing_read_host(bpr_ctx* c, double* avg_ms_host, int64_t* launches_host) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_timing_read_host: ctx is NULL");
  if (int rc = drain_timing(c)) return rc;
  if (avg_ms_host) *avg_ms_host = c->timed_launches ? c->timed_ms / (double)c->timed_launches : 0.0;
  if (launches_host) *launches_host = c->timed_launches;
  return BPR_OK;
}

}  // extern "C"
