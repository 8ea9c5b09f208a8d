// bpr_refresh.hip — AdaptiveSampler.update_stats on device: the snapshot's life cycle (buffers, cut, sort,
// swap) and the launches of the sort kernels (bpr_sort.h), as bpr_refresh_plan.h plans them.
// The device-wide route is ONE rocPRIM radix sort over composite
// 64-bit keys (factor << 32 | descending-orderable float bits), restricted to the 32 + log2(d)
// significant bits — measured 2.1x faster than DeviceSegmentedRadixSort / DeviceSegmentedSort for
// d = 128 segments of 20 k keys (tools/ubench/sort_bench.hip: 0.23 ms vs 0.49 ms).
#include <string.h>  // (rocprim's texture iterator calls the host memset)
#include <rocprim/rocprim.hpp>

#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "bpr_ctx_state.h"
#include "bpr_host.h"
#include "bpr_refresh_plan.h"
#include "bpr_sort.h"

namespace bpr {

// ---------------------------------------------------------------------------------------------
// Launches.  A kernel's ITEMS is a template argument and a column's length a runtime figure: with_items calls
// fn(std::integral_constant<int, N>) for the first N of its list that `items` fits (the last one otherwise).
// Every ladder names its own list — together they are the set of instantiations the library holds.
// ---------------------------------------------------------------------------------------------
template <int N, int... Rest, typename Fn>
static void with_items(int items, Fn&& fn) {
  if constexpr (sizeof...(Rest) == 0) fn(std::integral_constant<int, N>{});
  else if (items <= N) fn(std::integral_constant<int, N>{});
  else with_items<Rest...>(items, fn);
}

// what one refresh sorts (columns f_lo .. f_lo + nf of the keys just cut), where to, and on which stream
struct RefreshJob {
  int back, f_lo, nf;
  bool part;
  hipStream_t st;
  const float* keysT;  // (from here on: of column f_lo — the kernels index columns from 0)
  double* sig_acc;
  int32_t* order;
  float* sigma;
  int32_t* meta;
};

static void launch_sort_sub(bpr_ctx* c, hipStream_t st, int items, int nf, const float* keysT, double* sig_acc,
                            int32_t* order, float* sigma, int sub, int64_t len, float* keysA, int32_t* idsA,
                            const int32_t* only_flagged = nullptr) {
  with_items<6, 10, 12, 16, 20, 24, 28, 36>(items, [&](auto N) {
    hipLaunchKernelGGL((k_sort_sub<decltype(N)::value>), dim3(sub, nf), dim3(1024), 0, st, keysT, c->I, len, order,
                       keysA, idsA, sigma, sig_acc, only_flagged);
  });
}

template <int ITEMS>
static void launch_sort_flagged(bpr_ctx* c, const RefreshJob& j) {
  hipLaunchKernelGGL((k_sort_flagged<ITEMS>), dim3(j.nf), dim3(1024), 0, j.st, j.keysT, c->I, j.order, j.meta);
}

static void launch_sort_partial(bpr_ctx* c, const RefreshJob& j, int items) {
  with_items<6, 10, 12, 16, 20, 24>(items, [&](auto N) {
    hipLaunchKernelGGL((k_sort_partial<decltype(N)::value>), dim3(c->d), dim3(1024), 0, j.st, j.keysT, c->I,
                       j.order, j.sigma, j.meta, c->partial_target);
    launch_sort_flagged<decltype(N)::value>(c, j);
  });
}

static void launch_sort_binned(bpr_ctx* c, const RefreshJob& j, int items) {
  with_items<6, 10, 16, 20>(items, [&](auto N) {
    hipLaunchKernelGGL((k_sort_binned<decltype(N)::value>), dim3(j.nf), dim3(1024), 0, j.st, j.keysT, c->I, j.order,
                       j.sigma, j.meta);
    launch_sort_flagged<decltype(N)::value>(c, j);
  });
}

static int launch_sort_binned_split(bpr_ctx* c, const RefreshJob& j, const RefreshPlan& plan) {
  BPR_HIP_CHECK(hipMemsetAsync(j.meta, 0, sizeof(int32_t) * 2 * j.nf, j.st));  // a workgroup that gives up writes -1
  with_items<8, 12, 16, 20>(plan.sitems, [&](auto N) {
    constexpr int SITEMS = decltype(N)::value;
    if (plan.wide)  // 17-bit ids
      hipLaunchKernelGGL((k_sort_binned_split<SPLIT_WIDE + SITEMS>), dim3(plan.g, j.nf), dim3(1024), 0, j.st,
                         j.keysT, c->I, j.order, j.sigma, j.meta);
    else
      hipLaunchKernelGGL((k_sort_binned_split<SITEMS>), dim3(plan.g, j.nf), dim3(1024), 0, j.st, j.keysT, c->I,
                         j.order, j.sigma, j.meta);
  });
  return BPR_OK;
}

// the radix sort: `sub` workgroups per column and the merge levels behind them (only_flagged: of the columns
// the split binned sort flagged)
static void launch_sort_radix(bpr_ctx* c, const RefreshJob& j, int items, int sub, int64_t len,
                              const int32_t* only_flagged) {
  const int64_t I = c->I, n = (int64_t)c->d * I, foff = (int64_t)j.f_lo * I;
  float* keysA = reinterpret_cast<float*>(c->keys_sorted) + foff;
  int32_t* idsA = reinterpret_cast<int32_t*>(keysA + n);
  float* keysB = reinterpret_cast<float*>(idsA + n);
  int32_t* idsB = reinterpret_cast<int32_t*>(keysB + n);
  launch_sort_sub(c, j.st, items, j.nf, j.keysT, j.sig_acc, j.order, j.sigma, sub, len, keysA, idsA, only_flagged);
  int64_t run = len;
  for (int level = sub; level > 1; level /= 2, run *= 2) {
    const int last = level == 2;
    const int tiles_per_pair = (int)((2 * run + MERGE_TILE - 1) / MERGE_TILE);
    const unsigned mgrid = (unsigned)(((I + 2 * run - 1) / (2 * run)) * tiles_per_pair);
    hipLaunchKernelGGL(k_merge_runs, dim3(mgrid, j.nf), dim3(MERGE_THREADS), 0, j.st, keysA, idsA, I, run,
                       tiles_per_pair, keysB, last ? j.order : idsB, last, j.sigma, j.sig_acc, only_flagged);
    std::swap(keysA, keysB);
    std::swap(idsA, idsB);
  }
}

// device-wide sort: always every column (a sharded refresh is merely redundant here)
static int launch_sort_device(bpr_ctx* c, const RefreshJob& j) {
  const int64_t I = c->I, n = (int64_t)c->d * I, foff = (int64_t)j.f_lo * I;
  hipLaunchKernelGGL(k_sigma, dim3(c->d), dim3(256), 0, j.st, j.keysT - foff, I, j.sigma - j.f_lo);
  uint64_t* k64 = reinterpret_cast<uint64_t*>(c->keys_sorted);
  hipLaunchKernelGGL(k_compose_keys, dim3(2048), dim3(256), 0, j.st, j.keysT - foff, k64, n, I);
  int key_bits = 32;
  while ((1 << (key_bits - 32)) < c->d) ++key_bits;
  size_t bytes = c->sort_tmp_bytes;
  BPR_HIP_CHECK(rocprim::radix_sort_pairs(c->sort_tmp, bytes, k64, k64 + n, c->ids_in, j.order - foff, (int)n, 0,
                                          key_bits, j.st));
  return BPR_OK;
}

void refresh_free(bpr_ctx* c) {
  hot_free(c);
  heavy_free(c);
  hipFree(c->plan_keys);
  hipFree(c->plan_keys_sorted);
  hipFree(c->plan_tmp);
  c->plan_keys = c->plan_keys_sorted = nullptr;
  c->plan_tmp = nullptr;
  c->plan_cap = 0;
  if (c->side != nullptr) hipStreamSynchronize(c->side);
  hipFree(c->pc_keys); hipFree(c->pc_vals); hipFree(c->pc_tmp);
  hipFree(c->pc_keys2); hipFree(c->pc_vals2); hipFree(c->pc_cnt);
  c->pc_keys = c->pc_keys2 = nullptr; c->pc_vals = c->pc_vals2 = nullptr; c->pc_tmp = nullptr;
  c->pc_cnt = nullptr;
  c->pc_cap = 0;
  for (int k = 0; k < 2; ++k) {
    hipFree(c->order_alloc[k]);
    hipFree(c->sigma_buf[k]);
    c->order_alloc[k] = nullptr;
    c->sigma_buf[k] = nullptr;
  }
  for (int k = 0; k < 2; ++k) {
    hipFree(c->keysT_buf[k]);
    hipFree(c->sig_acc_buf[k]);
    hipFree(c->snap_meta[k]);
    c->keysT_buf[k] = nullptr;
    c->sig_acc_buf[k] = nullptr;
    c->snap_meta[k] = nullptr;
    c->snap_partial[k] = false;
    c->snap_keys[k] = nullptr;
  }
  c->meta_front = nullptr;
  c->keys_front = nullptr;
  hipFree(c->keys_sorted);
  hipFree(c->ids_in);
  hipFree(c->seg_offsets);
  c->sig_acc = nullptr;
  items_moved(c);  // (the key buffers are gone)
  hipFree(c->sort_tmp);
  c->order = nullptr;
  c->sigma = nullptr;
  c->keysT = c->keys_sorted = nullptr;
  c->ids_in = c->seg_offsets = nullptr;
  c->sort_tmp = nullptr;
  c->sort_tmp_bytes = 0;
  c->have_snapshot = false;
  split_refresh_done(c);
  c->part_pending = false;
}

void side_free(bpr_ctx* c) {  // bpr_ctx_destroy: the split refresh's events and (if ours) stream
  if (c->ev_keys) hipEventDestroy(c->ev_keys);
  if (c->ev_sorted) hipEventDestroy(c->ev_sorted);
  c->ev_keys = c->ev_sorted = nullptr;
  if (c->side_owned && c->side) hipStreamDestroy(c->side);
  c->side = nullptr;
  c->side_owned = false;
}

// The snapshot is taken in two steps.  CUT: k_transpose copies Q into the key buffer on the
// caller's stream — that instant is the snapshot's point in time.  SORT: the per-factor orders and
// sigma of those keys go to the BACK snapshot.  split = false: sort on the caller's stream and swap
// (AdaptiveSampler.update_stats as the reference calls it).  split = true
// (bpr_adaptive_refresh_begin): the sort runs on c->side behind an event, the caller's stream goes
// on — typically with the next STREAM launch, which is bound by the L2 atomic units and leaves the
// CUs mostly idle — and refresh_commit_impl (bpr_adaptive_refresh_commit) orders the swap.
int refresh_alloc(bpr_ctx* c) {
  const int64_t I = c->I;
  const int d = c->d;
  const int64_t n = (int64_t)d * I;
  if (n >= (int64_t)1 << 31) {
    set_error("bpr_adaptive_refresh: d*I must be < 2^31");
    return BPR_ERR_UNSUPPORTED;
  }
  if (I < 3) {
    set_error("bpr_adaptive_refresh: need at least 3 item rows");
    return BPR_ERR_INVALID;
  }
  if (c->order_alloc[0] != nullptr) return BPR_OK;
  for (int k = 0; k < 2; ++k) {
    BPR_HIP_CHECK(hipMalloc(&c->order_alloc[k], sizeof(int32_t) * (n + 2 * BPR_ORDER_PAD)));
    BPR_HIP_CHECK(hipMemsetAsync(c->order_alloc[k], 0, sizeof(int32_t) * (n + 2 * BPR_ORDER_PAD),
                                 c->stream));
    BPR_HIP_CHECK(hipMalloc(&c->sigma_buf[k], sizeof(float) * d));
  }
  for (int k = 0; k < 2; ++k) BPR_HIP_CHECK(hipMalloc(&c->snap_meta[k], sizeof(int32_t) * 2 * d));
  c->snap_front = 0;
  c->order = c->order_alloc[0] + BPR_ORDER_PAD;
  c->sigma = c->sigma_buf[0];
  for (int k = 0; k < 2; ++k) {
    BPR_HIP_CHECK(hipMalloc(&c->keysT_buf[k], sizeof(float) * n));
    BPR_HIP_CHECK(hipMalloc(&c->sig_acc_buf[k], sizeof(double) * 2 * d));
  }
  c->keys_w = 0;
  c->keysT = c->keysT_buf[0];
  c->sig_acc = c->sig_acc_buf[0];
  BPR_HIP_CHECK(hipMalloc(&c->keys_sorted, sizeof(uint64_t) * 2 * n));  // composite keys in|out
  BPR_HIP_CHECK(hipMalloc(&c->ids_in, sizeof(int32_t) * n));
  BPR_HIP_CHECK(hipMalloc(&c->seg_offsets, sizeof(int32_t) * (d + 1)));
  hipLaunchKernelGGL(k_iota, dim3(1024), dim3(256), 0, c->stream, c->ids_in, c->seg_offsets, I, d);
  size_t bytes = 0;
  uint64_t* k64 = reinterpret_cast<uint64_t*>(c->keys_sorted);
  BPR_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, k64, k64 + n, c->ids_in,
                                                   c->order, (int)n, 0, 64, c->stream));
  BPR_HIP_CHECK(hipMalloc(&c->sort_tmp, bytes > 0 ? bytes : 16));
  c->sort_tmp_bytes = bytes;
  return BPR_OK;
}

// the back snapshot becomes the front (keep_meta: a partial snapshot keeps its meta for the readers that walk it)
static void snapshot_to_front(bpr_ctx* c, int back, bool keep_meta) {
  c->snap_front = back;
  c->refresh_done = back;
  c->order = c->order_alloc[back] + BPR_ORDER_PAD;
  c->sigma = c->sigma_buf[back];
  c->meta_front = keep_meta && c->snap_partial[back] ? c->snap_meta[back] : nullptr;
  c->keys_front = c->snap_keys[back];
  front_replaced(c);
  c->have_snapshot = true;
}

static int back_snapshot(const bpr_ctx* c) { return c->have_snapshot ? (c->snap_front ^ 1) : c->snap_front; }

// ---- refresh_impl's steps
static int refresh_validate(bpr_ctx* c, bool split, int f_lo, int f_hi) {
  if (c->refresh_pending && !split && f_lo == 0 && f_hi == c->d) {
    // a lagged schedule ends every epoch with a split refresh in flight (StreamTrainer(refresh_lag=1));
    // whoever asks for a synchronous snapshot next — StrictTrainer, bpr_train_strict's refresh_every,
    // a plain bpr_adaptive_refresh — gets it: the pending one is committed first (its sort is waited
    // for, its buffers become the front pair) and the new snapshot then replaces it
    if (int rc = refresh_commit_impl(c)) return rc;
  }
  if (c->refresh_pending || c->part_pending) {
    set_error("bpr_adaptive_refresh: a split or sharded refresh is pending (bpr_adaptive_refresh_commit / "
              "_publish first)");
    return BPR_ERR_INVALID;
  }
  if (int rc = refresh_alloc(c)) return rc;
  if (f_lo < 0 || f_hi > c->d || f_lo >= f_hi) {
    set_error("bpr_adaptive_refresh_part: need 0 <= f_lo < f_hi <= d");
    return BPR_ERR_INVALID;
  }
  return BPR_OK;
}

// cut (unless the last STREAM launch's epilogue did it: bpr_train_stream_cut); *event_on_cut: ev_keys rode on
// the cut kernel.  Hands the job the buffers just cut; the next cut goes to the other pair.
static int refresh_cut(bpr_ctx* c, bool split, RefreshJob* j, bool* event_on_cut) {
  const int64_t I = c->I;
  *event_on_cut = c->keys_cut && c->keys_event;
  if (!c->keys_cut) {
    dim3 tgrid((unsigned)((I + 31) / 32), (unsigned)((c->d + 31) / 32));
    hipLaunchKernelGGL(k_transpose, tgrid, dim3(256), 0, c->stream, c->Q, c->keysT, I, c->d, c->sig_acc);
  }
  if (c->keys_cut && c->keys_on_side && !split) {
    // the keys were cut on the side stream (bpr_train_stream_acut) and this sort runs on the launch
    // stream: order it behind that cut (the split sort waits for ev_keys on the side stream anyway)
    BPR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_keys, 0));
    acut_waited(c);
  }
  keys_consumed(c);
  j->keysT = c->keysT + (int64_t)j->f_lo * I;
  j->sig_acc = c->sig_acc + 2 * j->f_lo;
  c->keys_w ^= 1;
  c->keysT = c->keysT_buf[c->keys_w];
  c->sig_acc = c->sig_acc_buf[c->keys_w];
  return BPR_OK;
}

// the stream the sort runs on: the caller's, or — split — c->side behind the cut's event
static int refresh_stream(bpr_ctx* c, bool split, bool event_on_cut, hipStream_t* st) {
  *st = c->stream;
  if (!split) return BPR_OK;
  if (c->side == nullptr) {
    BPR_HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    c->side_owned = true;
  }
  if (c->ev_keys == nullptr) {
    BPR_HIP_CHECK(hipEventCreateWithFlags(&c->ev_keys, hipEventDisableTiming));
    BPR_HIP_CHECK(hipEventCreateWithFlags(&c->ev_sorted, hipEventDisableTiming));
  }
  if (!event_on_cut) BPR_HIP_CHECK(hipEventRecord(c->ev_keys, c->stream));
  BPR_HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_keys, 0));
  *st = c->side;
  return BPR_OK;
}

// which sorter, how many workgroups per column, which instantiations: bpr_refresh_plan.h
static RefreshPlan refresh_plan_for(bpr_ctx* c, bool split, const RefreshJob& j) {
  static const bool no_fast = getenv("BPR_NO_FAST_REFRESH") != nullptr;  // (process-wide test aids, read once)
  RefreshShape shape = {};
  shape.I = c->I; shape.nf = j.nf; shape.split = split; shape.part = j.part;
  shape.tune_binned = c->tune_binned; shape.tune_binned_split = c->tune_binned_split;
  shape.tune_refresh_sub = c->tune_refresh_sub;  // bpr_set_tuning("refresh_sub", ...): tests force the split / merge paths on small tables
  shape.tune_partial = c->tune_partial; shape.no_fast = no_fast;
  const RefreshPlan plan = plan_refresh(shape);
  bpr_ctx::RefreshInfo& ri = c->refresh_info[j.back];
  ri.route = plan.route; ri.g = plan.g; ri.sub = plan.sub; ri.f_lo = j.f_lo; ri.nf = j.nf;
  ri.items = plan.route == REFRESH_BINNED_SPLIT ? plan.sitems : plan.items;
  c->snap_partial[j.back] = plan.partial;
  c->snap_keys[j.back] = j.keysT;
  return plan;
}

static int refresh_launch(bpr_ctx* c, const RefreshPlan& plan, const RefreshJob& j) {
  if (plan.partial) {
    launch_sort_partial(c, j, plan.items);
  } else if (plan.route == REFRESH_BINNED) {
    launch_sort_binned(c, j, plan.items);
  } else {
    // the radix path: every column, or — behind the split binned sort — the columns it flagged
    const int32_t* only_flagged = nullptr;
    if (plan.route == REFRESH_BINNED_SPLIT) {
      if (int rc = launch_sort_binned_split(c, j, plan)) return rc;
      BPR_HIP_CHECK(hipGetLastError());
      only_flagged = j.meta;
    }
    if (plan.fallback == REFRESH_FB_FLAGGED) {  // a flagged column fits one workgroup: k_sort_flagged
      with_items<10, 20, 28, 36>(plan.fb_items, [&](auto N) { launch_sort_flagged<decltype(N)::value>(c, j); });
    } else if (plan.route == REFRESH_RADIX || plan.fallback == REFRESH_FB_RADIX) {
      launch_sort_radix(c, j, plan.route == REFRESH_RADIX ? plan.items : plan.fb_items, plan.sub, plan.len,
                        only_flagged);
    } else if (plan.route == REFRESH_DEVICE) {
      if (int rc = launch_sort_device(c, j)) return rc;
    }
  }
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

int refresh_impl(bpr_ctx* c, bool split, int f_lo, int f_hi) {
  if (int rc = refresh_validate(c, split, f_lo, f_hi)) return rc;
  // f_lo .. f_hi: the factors (columns) this call sorts — all of them, or this rank's share of a
  // refresh sharded over the ranks of a multi-GPU job (bpr_adaptive_refresh_part: the caller
  // gathers the other columns into the back snapshot and publishes it)
  RefreshJob j = {};
  j.back = back_snapshot(c);
  j.f_lo = f_lo;
  j.nf = f_hi - f_lo;
  j.part = f_lo != 0 || f_hi != c->d;
  j.order = c->order_alloc[j.back] + BPR_ORDER_PAD + (int64_t)f_lo * c->I;
  j.sigma = c->sigma_buf[j.back] + f_lo;
  j.meta = c->snap_meta[j.back] + 2 * f_lo;
  bool event_on_cut = false;
  if (int rc = refresh_cut(c, split, &j, &event_on_cut)) return rc;
  if (int rc = refresh_stream(c, split, event_on_cut, &j.st)) return rc;
  const RefreshPlan plan = refresh_plan_for(c, split, j);
  if (int rc = refresh_launch(c, plan, j)) return rc;
  if (j.part) {  // the caller fills the other columns and publishes (refresh_publish_impl)
    c->part_pending = true;
  } else if (split) {
    BPR_HIP_CHECK(hipEventRecord(c->ev_sorted, c->side));
    split_refresh_queued(c);
  } else {
    snapshot_to_front(c, j.back, true);
  }
  return BPR_OK;
}

// A partial front snapshot sorted whole, in place, from the keys it was cut from: for every reader but
// k_stream (the sampler kernels behind the Python API, the batched STREAM kernel, bpr_adaptive_get_snapshot).
int snapshot_complete_impl(bpr_ctx* c) {
  if (c->meta_front == nullptr || !c->have_snapshot) return BPR_OK;
  if (c->keys_front_stale) {
    // the lag-1 pipeline's next cut writes the buffer this partial front was sorted from (the launch that
    // read the front is over by then); completing it now would sort NEWER keys into an order k_stream never walked
    set_error("the partial snapshot in front can no longer be completed: a later cut (bpr_train_stream_cut / _acut) "
              "overwrote the keys it was sorted from — commit the pending refresh (bpr_adaptive_refresh_commit) or "
              "refresh again before sampling through the API");
    return BPR_ERR_INVALID;
  }
  const int front = c->snap_front;
  const int64_t len = (c->I + 15) / 16 * 16;
  // (sig_acc is unused by the single-workgroup form)
  launch_sort_sub(c, c->stream, (int)((len + 1023) / 1024), c->d, c->keys_front, c->sig_acc,
                  c->order_alloc[front] + BPR_ORDER_PAD, c->sigma_buf[front], 1, len, nullptr, nullptr);
  BPR_HIP_CHECK(hipGetLastError());
  c->snap_partial[front] = false;
  c->meta_front = nullptr;
  return BPR_OK;
}

int refresh_publish_impl(bpr_ctx* c) {
  if (!c->part_pending) {
    set_error("bpr_adaptive_refresh_publish: no sharded refresh is pending");
    return BPR_ERR_INVALID;
  }
  snapshot_to_front(c, back_snapshot(c), false);  // (a sharded refresh is always sorted whole)
  c->part_pending = false;
  return BPR_OK;
}

int refresh_commit_impl(bpr_ctx* c) {
  if (!c->refresh_pending) {
    set_error("bpr_adaptive_refresh_commit: no split refresh is pending");
    return BPR_ERR_INVALID;
  }
  BPR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_sorted, 0));
  snapshot_to_front(c, back_snapshot(c), true);
  split_refresh_done(c);
  return BPR_OK;
}

// What the last completed refresh ran (bpr_adaptive_refresh_info): the plan's figures as refresh_impl recorded them,
// and the columns the split binned sort flagged, read back from its meta — memset to 0 before the launch; a
// workgroup that gives up writes -1, which the radix fallback leaves and k_sort_flagged replaces by I.
int refresh_info_impl(bpr_ctx* c, int32_t* info_host) {
  for (int k = 0; k < BPR_REFRESH_INFO_LEN; ++k) info_host[k] = -1;
  if (c->refresh_done < 0) return BPR_OK;  // no refresh yet: every field -1
  const bpr_ctx::RefreshInfo& ri = c->refresh_info[c->refresh_done];
  info_host[0] = ri.route;
  info_host[1] = ri.g;
  info_host[2] = ri.items;
  info_host[3] = ri.sub;
  if (ri.route == REFRESH_BINNED_SPLIT) {
    BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<int32_t> meta(2 * (size_t)ri.nf);
    BPR_HIP_CHECK(hipMemcpy(meta.data(), c->snap_meta[c->refresh_done] + 2 * ri.f_lo, sizeof(int32_t) * meta.size(),
                            hipMemcpyDeviceToHost));
    int flagged = 0;
    for (int f = 0; f < ri.nf; ++f) flagged += meta[2 * (size_t)f] != 0 ? 1 : 0;
    info_host[4] = flagged;
  }
  return BPR_OK;
}

}  // namespace bpr

using namespace bpr;
extern "C" {

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

}  // extern "C"
