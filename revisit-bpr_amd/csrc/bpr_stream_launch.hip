// bpr_stream_launch.hip — the STREAM launch (as bpr_stream_plan.h plans it), its three epilogue forms, and
// bpr_sync_cut, which shares the cut with them.  At the end: the stand-alone samplers (k_sample).  They share the
// uniform draw's device code with k_stream, and the compiler shapes that code by all of its callers in one object:
// apart, 36 uniform k_stream instantiations come out one instruction different (profiles/bprcore_split_resources.md).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "bpr_ctx_state.h"
#include "bpr_host.h"
#include "bpr_kernels.h"
#include "bpr_opt_plan.h"
#include "bpr_stream_kernels.h"
#include "bpr_stream_plan.h"

namespace bpr {
static_assert(ORDER_PAD == BPR_ORDER_PAD, "walk vector width vs snapshot padding");
static_assert(SEEN_CSR == STREAM_SEEN_CSR && SEEN_BITMAP == STREAM_SEEN_BITMAP && SEEN_LIST == STREAM_SEEN_LIST &&
                  NEG_GIVEN == BPR_NEG_GIVEN && NEG_DYNAMIC == BPR_NEG_DYNAMIC && NEG_WARP == BPR_NEG_WARP,
              "the launch plan names the kernels' template arguments");

// STREAM grids (bpr_stream_plan.h): BPR_MAX_BLOCKS caps them (experiments).
static int64_t stream_grid_cap() {
  static const bool forced = getenv("BPR_MAX_BLOCKS") != nullptr;
  return forced ? (int64_t)max_blocks() : STREAM_MAX_GRID;
}

int sum_partials(bpr_ctx* c, const float* partials, int n_blocks, float* out) {
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, partials, n_blocks, out);
  BPR_HIP_CHECK(hipGetLastError());
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
  hot_block_folded(c);
  if (c->hot_H <= 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->ev_keys != nullptr) BPR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_keys, 0));
  acut_waited(c);
  return stream_epilogue(c, nullptr, 0, nullptr, true, false, nullptr);  // (Q + delta is what it was: keys cut from it stay valid)
}

// bpr_train_stream_cut under the hot tier leaves its loss partials to the bpr_sync_cut that should
// follow.  Whoever comes first instead — the next launch (it overwrites the partials), a hot exchange
// of the three-call protocol (bpr_hot_exchange / bpr_hot_sync), the end of the tier — sums them now.
int flush_deferred_stats(bpr_ctx* c) {
  if (!c->defer_pending) return BPR_OK;
  float* out = c->defer_out;
  stats_taken(c);
  if (out == nullptr || c->defer_blocks <= 0) return BPR_OK;
  BPR_HIP_CHECK(hipSetDevice(c->device));
  return sum_partials(c, c->dev_scalars, c->defer_blocks, out);
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
    acut_waited(c);
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
    if (bias_wide_refill_needed(c))
      hipLaunchKernelGGL(k_bias_widen, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream, c->bias,
                         c->bias_w, (int32_t)c->I);
    bias_wide_taken(c);
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
  if (hot && c->hot_tier) launch_left_hot_deltas(c);  // this launch's deltas stay in the block for bpr_hot_exchange
  if (a.bias != nullptr && !bias_in_epilogue)
    hipLaunchKernelGGL(k_bias_narrow, dim3((unsigned)((c->I + 255) / 256)), dim3(256), 0, c->stream,
                       c->bias_w, c->bias, (int32_t)c->I);
  if (a.bias != nullptr) bias_wide_synced(c);

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
    keys_were_cut(c, true, true);
    if (!acut_fold) acut_left_unfolded(c, hot);
    return BPR_OK;
  }
  if (defer) {
    stats_deferred(c, (int)p.grid, out_scalars);
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
    keys_were_cut(c, ride, false);
  } else if (out_scalars != nullptr || fold || bias_in_epilogue) {
    return stream_epilogue(c, a.partials, (int)p.grid, out_scalars, fold, bias_in_epilogue, nullptr);
  }
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}


}  // namespace bpr

using namespace bpr;
extern "C" {

static int train_stream_impl(bpr_ctx* c, const int32_t* users, const int32_t* pos, int32_t* neg,
                             int64_t n, int32_t sampler, float adaptive_p, uint64_t seed,
                             uint64_t offset, int64_t max_inflight, float* out_scalars, bool cut,
                             bool acut = false) {
  if (acut)  // (no snapshot to cut)
    if (int rc = refuse_scored("bpr_train_stream_acut", sampler)) return rc;
  // (check_bound folds pending hot deltas for everybody but the acut pipeline itself)
  if (int rc = check_triples(c, "bpr_train_stream", users, pos, n, !acut)) return rc;
  items_moved(c);  // (the bias: launch_stream keeps the wide table's books itself)
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
  stats_taken(c);
  hot_block_cut(c);  // (the hot-tier step cut the block)
  keys_were_cut(c, true, false, false);  // the next bpr_adaptive_refresh_begin only queues the sort
  return BPR_OK;
}

int bpr_stream_lds_rows(bpr_ctx* c) {
  return c == nullptr ? 0 : c->last_lds_rows;
}

int bpr_stream_run_len(bpr_ctx* c) {
  return c == nullptr ? 0 : c->last_run_len;
}

}  // extern "C"

// ---- the stand-alone samplers behind the Python API (k_sample) -----------------------------------------------------
namespace bpr {

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

// (the sampler kernels read a snapshot sorted whole: the callers complete a partial one first)
static SampleArgs sample_args(const bpr_ctx* c) {
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P; a.I = c->I; a.d = c->d;
  a.indptr = c->indptr; a.indices = c->indices;
  a.order = c->order; a.sigma = c->sigma;
  a.iw = ItemWeights{c->w_accept, c->w_alias};
  a.mP = c->mP; a.vP = c->vP; a.lastP = opt_kind_lazy(c->opt_kind) ? c->lastP : nullptr;
  a.o = opt_dev(c, c->step + 1);
  return a;
}

}  // namespace bpr

using namespace bpr;
extern "C" {

int bpr_sample_uniform(bpr_ctx* c, const int32_t* users, int64_t B, uint64_t seed, uint64_t offset,
                       int32_t* neg_out) {
  if (int rc = check_bound(c, "bpr_sample_uniform")) return rc;
  if (c->indptr == nullptr) return fail(BPR_ERR_INVALID, "bpr_sample_uniform: seen CSR not bound");
  if (users == nullptr || neg_out == nullptr || B < 0)
    return fail(BPR_ERR_INVALID, "bpr_sample_uniform: bad argument");
  if (int rc = snapshot_complete_impl(c)) return rc;
  SampleArgs a = sample_args(c);
  a.users = users; a.n = B; a.seed = seed; a.offset = offset; a.neg = neg_out;
  return launch_sample(c, SAMPLE_UNIFORM, a);
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
  if (int rc = snapshot_complete_impl(c)) return rc;
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
  if (int rc = snapshot_complete_impl(c)) return rc;
  SampleArgs a = sample_args(c);
  a.users = users; a.factor_in = factor; a.rank_in = rank; a.n = B; a.neg = neg_out;
  return launch_sample(c, SAMPLE_PICK, a);
}

}  // extern "C"
