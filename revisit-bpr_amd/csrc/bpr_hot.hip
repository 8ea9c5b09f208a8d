// bpr_hot.hip — what is built once per training set or seen CSR: the hot-item list with its delta block
// (bpr_set_hot_items, the STREAM kernel's replica rows) and the heavy users' seen bitmaps; at the end, the entry
// points of the hot block, the hot tier and the item reconciliation passes (bpr_hot_kernels.h).
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bpr_ctx_state.h"
#include "bpr_host.h"
#include "bpr_hot_kernels.h"

namespace bpr {

// ---------------------------------------------------------------------------------------------
// Hot item rows: popularity of the training positives -> the H most popular rows get replica
// delta rows for their STREAM updates (same-line atomic contention on the few
// hundred hot lines is what sets the kernel's floor on popularity-skewed data).
// ---------------------------------------------------------------------------------------------
__global__ void k_item_hist(const int32_t* __restrict__ pos, int64_t n, int64_t I,
                            uint32_t* __restrict__ counts) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int32_t it = pos[k];
    if (it >= 0 && it < I) atomicAdd(&counts[it], 1u);
  }
}
void hot_free(bpr_ctx* c) {
  hipFree(c->hot_slot);
  hipFree(c->hot_items);
  hipFree(c->hot_delta_alloc);
  hipFree(c->hot_canon);
  hipFree(c->hot_code);
  hipFree(c->hot_by_rank);
  c->hot_canon = c->hot_code = c->hot_by_rank = nullptr;
  c->hot_explicit = false;
  c->hot_tier = false;
  hot_block_cut(c);
  c->hot_delta_alloc = nullptr;
  c->hot_slot = c->hot_items = nullptr;
  c->hot_delta = nullptr;
  c->hot_H = c->hot_R = 0;
  c->hot_key_ptr = nullptr;
  c->hot_key_n = 0;
}

// Channel model behind the slot assignment (tools/ubench/atomic_bench.hip): memory
// is interleaved over HOT_CHANNELS channels in HOT_GRANULE-byte units, a row update sends one
// atomic request per 128-byte line, and a STREAM launch lasts as long as its most loaded channel
// (uniform popularity 0.185 ms; max/mean channel load 1.12 -> 0.207 ms, 1.455 -> 0.27 ms).
constexpr int HOT_CHANNELS = 128;
constexpr int64_t HOT_GRANULE = 256;
static inline int channel_of(uint64_t byte_addr) {
  return (int)((byte_addr / HOT_GRANULE) % HOT_CHANNELS);
}

// The H most popular rows take their STREAM updates in the delta block.  Which SLOT a row gets
// decides which channels carry its load: the rows are placed greedily, heaviest first, each into
// the free slot whose channels end up least loaded — counting the load the rows left in Q put on
// every channel — so the block evens out the whole launch, not only itself.
// cnt: positives per item (the channel model's load; may be all zero for a given hot set);
// given != NULL: the hot set, in the caller's canonical order (bpr_set_hot_items).
static int hot_build_from(bpr_ctx* c, std::vector<uint32_t>& cnt, const int32_t* given, int H, int64_t n) {
  const int64_t I = c->I;
  const int R = c->hot_reps_opt > 0 ? c->hot_reps_opt : 1;
  std::vector<int32_t> by((size_t)I);
  if (given != nullptr) {
    for (int k = 0; k < H; ++k) by[k] = given[k];
  } else {
    // the H most popular rows (ties by ascending id; the pad row and rows nobody likes stay out)
    for (int64_t i = 0; i < I; ++i) by[i] = (int32_t)i;
    if (c->pad_item >= 0 && c->pad_item < I) cnt[c->pad_item] = 0;
    std::partial_sort(by.begin(), by.begin() + H, by.end(), [&](int32_t x, int32_t y) {
      return cnt[x] != cnt[y] ? cnt[x] > cnt[y] : x < y;
    });
    while (H > 0 && cnt[by[H - 1]] == 0) --H;
  }
  if (H == 0) return BPR_OK;
  // the block starts on a channel-round boundary so that slot -> channels is known
  const size_t round_bytes = (size_t)HOT_CHANNELS * HOT_GRANULE;
  const size_t block_bytes = sizeof(float) * (size_t)R * H * c->d;
  BPR_HIP_CHECK(hipMalloc(&c->hot_delta_alloc, block_bytes + round_bytes));
  c->hot_delta = reinterpret_cast<float*>(((uintptr_t)c->hot_delta_alloc + round_bytes - 1) /
                                          round_bytes * round_bytes);
  BPR_HIP_CHECK(hipMemsetAsync(c->hot_delta, 0, block_bytes, c->stream));
  const int64_t row_bytes = (int64_t)c->d * 4;
  const int lines = (int)((row_bytes + 127) / 128);
  // expected line requests per row and launch: its positives, plus the negatives — close to
  // uniform over the items under both samplers (profiles/r03_neg_hist.txt)
  const double neg_share = (double)n / (double)(I - 1);
  std::vector<char> is_hot((size_t)I, 0);
  for (int k = 0; k < H; ++k) is_hot[by[k]] = 1;
  double load[HOT_CHANNELS] = {0.0};
  const uint64_t qbase = (uint64_t)(uintptr_t)c->Q;
  for (int64_t i = 1; i < I; ++i) {
    if (is_hot[i]) continue;
    const double w = (double)cnt[i] + neg_share;
    for (int l = 0; l < lines; ++l) load[channel_of(qbase + (uint64_t)(i * row_bytes + l * 128))] += w;
  }
  // placement order: heaviest first (a given set need not be sorted by popularity)
  std::vector<int> place((size_t)H);
  for (int k = 0; k < H; ++k) place[k] = k;
  std::stable_sort(place.begin(), place.end(), [&](int x, int y) { return cnt[by[x]] > cnt[by[y]]; });
  std::vector<int32_t> slot_of((size_t)I, -1), item_of((size_t)H, -1), canon_of((size_t)H, -1);
  std::vector<int32_t> code_of((size_t)I, -1), by_rank((size_t)H, -1);  // LDS tier: rank = placement order, heaviest first
  std::vector<char> used((size_t)H, 0);
  const uint64_t hbase = (uint64_t)(uintptr_t)c->hot_delta;
  static const bool naive = getenv("BPR_HOT_NAIVE") != nullptr;  // measurement aid: slot = rank
  // (the greedy search is H^2 slot evaluations: beyond 4,096 rows the block is filled in order —
  // that many rows even out over the channels by themselves)
  const bool in_order = naive || H > 4096;
  for (int kk = 0; kk < H; ++kk) {
    const int k = place[kk];
    const int32_t it = by[k];
    const double w = (double)cnt[it] + neg_share;
    int best = -1;
    double best_cost = 0.0;
    for (int s = 0; s < H && !in_order; ++s) {
      if (used[s]) continue;
      double cost = 0.0;  // the most loaded channel among the slot's lines, after the row moved in
      for (int l = 0; l < lines; ++l)
        cost = std::max(cost, load[channel_of(hbase + (uint64_t)(s * row_bytes + l * 128))] + w);
      if (best < 0 || cost < best_cost) {
        best = s;
        best_cost = cost;
      }
    }
    if (in_order) best = kk;
    used[best] = 1;
    slot_of[it] = best;
    item_of[best] = it;
    canon_of[best] = k;
    if (H < 32768) code_of[it] = (int32_t)(((uint32_t)kk << 16) | (uint32_t)best);
    by_rank[kk] = best;
    for (int l = 0; l < lines; ++l)
      load[channel_of(hbase + (uint64_t)(best * row_bytes + l * 128))] += w;
  }
  {
    double mx = 0.0, sum = 0.0;
    for (double v : load) {
      mx = std::max(mx, v);
      sum += v;
    }
    c->hot_balance = sum > 0.0 ? mx / (sum / HOT_CHANNELS) : 1.0;
    if (getenv("BPR_HOT_VERBOSE"))
      fprintf(stderr, "[bprcore] hot block: %d rows, modelled channel load max/mean = %.3f\n", H,
              c->hot_balance);
  }
  BPR_HIP_CHECK(hipMalloc(&c->hot_slot, sizeof(int32_t) * I));
  BPR_HIP_CHECK(hipMalloc(&c->hot_items, sizeof(int32_t) * H));
  BPR_HIP_CHECK(hipMalloc(&c->hot_canon, sizeof(int32_t) * H));
  BPR_HIP_CHECK(hipMemcpyAsync(c->hot_slot, slot_of.data(), sizeof(int32_t) * I,
                               hipMemcpyHostToDevice, c->stream));
  BPR_HIP_CHECK(hipMemcpyAsync(c->hot_items, item_of.data(), sizeof(int32_t) * H,
                               hipMemcpyHostToDevice, c->stream));
  BPR_HIP_CHECK(hipMemcpyAsync(c->hot_canon, canon_of.data(), sizeof(int32_t) * H,
                               hipMemcpyHostToDevice, c->stream));
  if (H < 32768) {
    BPR_HIP_CHECK(hipMalloc(&c->hot_code, sizeof(int32_t) * I));
    BPR_HIP_CHECK(hipMalloc(&c->hot_by_rank, sizeof(int32_t) * H));
    BPR_HIP_CHECK(hipMemcpyAsync(c->hot_code, code_of.data(), sizeof(int32_t) * I, hipMemcpyHostToDevice, c->stream));
    BPR_HIP_CHECK(hipMemcpyAsync(c->hot_by_rank, by_rank.data(), sizeof(int32_t) * H, hipMemcpyHostToDevice,
                                 c->stream));
  }
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));  // the host vectors go out of scope
  c->hot_H = H;
  c->hot_R = R;
  return BPR_OK;
}

int hot_build_impl(bpr_ctx* c, const int32_t* pos, int64_t n) {
  if (c->hot_explicit) {  // the caller's hot set stays (bpr_set_hot_items); only note the training set
    c->hot_key_ptr = pos;
    c->hot_key_n = n;
    return BPR_OK;
  }
  hot_free(c);
  const int64_t I = c->I;
  int H = c->hot_rows_opt;
  if (H > I - 1) H = (int)(I - 1);
  c->hot_key_ptr = pos;
  c->hot_key_n = n;
  if (H <= 0 || c->hot_reps_opt <= 0 || n <= 0) return BPR_OK;
  uint32_t* counts = nullptr;
  BPR_HIP_CHECK(hipMalloc(&counts, sizeof(uint32_t) * I));
  BPR_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(uint32_t) * I, c->stream));
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_item_hist, dim3(grid), dim3(256), 0, c->stream, pos, n, I, counts);
  std::vector<uint32_t> cnt((size_t)I);
  BPR_HIP_CHECK(hipMemcpyAsync(cnt.data(), counts, sizeof(uint32_t) * I, hipMemcpyDeviceToHost,
                               c->stream));
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));  // one-time setup per training set
  hipFree(counts);
  return hot_build_from(c, cnt, nullptr, H, n);
}

// bpr_set_hot_items: the hot set as the caller gives it (the ranks of a multi-GPU job agree on it);
// counts (per item, may be NULL) only steer the slot placement.
int hot_set_items_impl(bpr_ctx* c, const int32_t* items, int H, const uint32_t* counts) {
  const void* key_ptr = c->hot_key_ptr;
  const int64_t key_n = c->hot_key_n;
  hot_free(c);
  c->hot_key_ptr = (const int32_t*)key_ptr;
  c->hot_key_n = key_n;
  c->hot_explicit = H > 0;
  if (H <= 0) return BPR_OK;
  std::vector<uint32_t> cnt((size_t)c->I, 0u);
  int64_t n = 0;
  if (counts != nullptr)
    for (int64_t i = 0; i < c->I; ++i) {
      cnt[i] = counts[i];
      n += counts[i];
    }
  if (c->hot_reps_opt <= 0) c->hot_reps_opt = 1;
  return hot_build_from(c, cnt, items, H, n > 0 ? n : 1);
}

// ---------------------------------------------------------------------------------------------
// Heavy users' seen bitmaps (bpr_device.h SeenBitmap / SeenList): users with more than T seen
// items get an I-bit row in HBM, filled once per seen CSR.
// ---------------------------------------------------------------------------------------------
__global__ void k_heavy_mark(const int64_t* __restrict__ indptr, int64_t U, int T, uint32_t words,
                             uint32_t* __restrict__ off, uint32_t* __restrict__ counter) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < U;
       u += (int64_t)gridDim.x * blockDim.x) {
    const int64_t cnt = indptr[u + 1] - indptr[u];
    off[u] = cnt > (int64_t)T ? atomicAdd(counter, 1u) * words : 0xFFFFFFFFu;
  }
}
__global__ void k_heavy_fill(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                             int64_t U, const uint32_t* __restrict__ off,
                             uint32_t* __restrict__ bits) {
  for (int64_t u = blockIdx.x; u < U; u += gridDim.x) {  // a block per user (the few heavy ones work)
    const uint32_t o = off[u];
    if (o == 0xFFFFFFFFu) continue;
    const int64_t lo = indptr[u], hi = indptr[u + 1];
    for (int64_t k = lo + threadIdx.x; k < hi; k += blockDim.x) {
      const int32_t it = indices[k];
      atomicOr(&bits[o + (uint32_t)(it >> 5)], 1u << (it & 31));
    }
  }
}

void heavy_free(bpr_ctx* c) {
  hipFree(c->heavy_off);
  hipFree(c->heavy_bits);
  c->heavy_off = c->heavy_bits = nullptr;
  c->heavy_n = 0;
  c->heavy_for = nullptr;
}

int heavy_build_impl(bpr_ctx* c) {
  if (c->heavy_for == c->indptr) return BPR_OK;
  heavy_free(c);
  c->heavy_for = c->indptr;
  int T = c->heavy_T_opt;  // bpr_set_heavy_users (-1 = no heavy table)
  if (T < 0 || c->indptr == nullptr) return BPR_OK;
  const uint32_t words = (uint32_t)(((c->I + 31) / 32 + 3) / 4 * 4);
  uint32_t* counter = nullptr;
  BPR_HIP_CHECK(hipMalloc(&counter, sizeof(uint32_t)));
  BPR_HIP_CHECK(hipMalloc(&c->heavy_off, sizeof(uint32_t) * c->U));
  const unsigned grid = (unsigned)std::min<int64_t>((c->U + 255) / 256, 2048);
  uint32_t n_heavy = 0;
  for (;;) {  // at most 2^31 words (8 GB) of bitmaps: raise the threshold until they fit
    BPR_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_heavy_mark, dim3(grid), dim3(256), 0, c->stream, c->indptr, c->U, T, words,
                       c->heavy_off, counter);
    BPR_HIP_CHECK(hipMemcpyAsync(&n_heavy, counter, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                 c->stream));
    BPR_HIP_CHECK(hipStreamSynchronize(c->stream));  // one-time setup per seen CSR
    // the bitmaps must fit the cap (bpr_set_heavy_users; at most 2^31 words): raise the threshold
    // until they do
    const uint64_t cap_words = std::min<uint64_t>((uint64_t)1 << 31, (uint64_t)c->heavy_max_bytes / 4);
    if ((uint64_t)n_heavy * words < cap_words) break;
    T = T > 0 ? T * 2 : 1;
  }
  hipFree(counter);
  c->heavy_T = T;
  c->heavy_n = n_heavy;
  if (n_heavy == 0) {
    hipFree(c->heavy_off);
    c->heavy_off = nullptr;
    return BPR_OK;
  }
  const size_t bytes = sizeof(uint32_t) * (size_t)n_heavy * words;
  BPR_HIP_CHECK(hipMalloc(&c->heavy_bits, bytes));
  BPR_HIP_CHECK(hipMemsetAsync(c->heavy_bits, 0, bytes, c->stream));
  hipLaunchKernelGGL(k_heavy_fill, dim3((unsigned)std::min<int64_t>(c->U, 65535)), dim3(256), 0,
                     c->stream, c->indptr, c->indices, c->U, c->heavy_off, c->heavy_bits);
  BPR_HIP_CHECK(hipGetLastError());
  if (getenv("BPR_HOT_VERBOSE"))
    fprintf(stderr, "[bprcore] heavy users (> %d seen items): %u, %.1f MB of bitmaps\n", T, n_heavy,
            bytes / 1e6);
  return BPR_OK;
}

// one elementwise pass of the item reconciliation over n elements of the four tables, on the caller's stream
template <typename K, typename... A>
static int item_pass(const char* who, const void* q, const void* base, const void* own, const void* tot, int64_t n,
                     void* hip_stream, K kernel, A... args) {
  if (n < 0 || (n > 0 && (!q || !base || !own || !tot))) return fail(BPR_ERR_INVALID, std::string(who) + ": bad argument");
  if (n == 0) return BPR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 1023) / 1024, 4096);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, args...);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

}  // namespace bpr

using namespace bpr;
extern "C" {

int bpr_item_delta(const float* q, const float* base, float* own, float* tot, int64_t n, void* hip_stream) {
  return item_pass("bpr_item_delta", q, base, own, tot, n, hip_stream, k_item_delta, q, base, own, tot, n);
}

int bpr_item_fold(float* q, float* base, const float* own, const float* tot, float scale, int32_t rebase, int64_t n,
                  void* hip_stream) {
  return item_pass("bpr_item_fold", q, base, own, tot, n, hip_stream, k_item_fold, q, base, own, tot, scale, rebase, n);
}

int bpr_item_fold_delta(float* q, float* base, float* own, float* tot, float scale, int64_t n, void* hip_stream) {
  return item_pass("bpr_item_fold_delta", q, base, own, tot, n, hip_stream, k_item_fold_delta, q, base, own, tot, scale, n);
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
  items_moved(c);  // (moves only hot item rows, no bias)
  HotStepArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = c->Q; a.delta = c->hot_delta; a.hot_items = c->hot_items; a.canon = c->hot_canon;
  a.hb = hot_base; a.tot = tot; a.cold_base = cold_base;
  a.H = c->hot_H; a.R = c->hot_R; a.d = c->d; a.fold_prev = fold_prev != 0; a.cut = cut != 0;
  const int64_t n = (int64_t)c->hot_H * c->d;
  hipLaunchKernelGGL(k_hot_step, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0,
                     c->stream, a);
  BPR_HIP_CHECK(hipGetLastError());
  if (cut) hot_block_cut(c);  // the block is zero again: the next launch may take the LDS tier
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

}  // extern "C"
