// bpr_sort.h — the adaptive snapshot's sort kernels (included by bpr_refresh.hip, which launches them).
// (reference: revisit_bpr/modules/neg_samplers.py:126-132; experiments/bpr/exp.py:344-354).
//
// The reference snapshots Qᵀ [d, I] and, at every sample, argsorts one masked row of it.  The only
// thing those argsorts ever use of the snapshot is each factor's ORDER of the items, so the
// snapshot kept here is order[f][:] = argsort_desc(Q[:, f]) (stable, ties by item id) plus
// sigma_f = unbiased std of Q[1:, f].  Four sorters make it, chosen by bpr_refresh_plan.h: the radix sort
// (k_sort_sub, k_merge_runs), the partial sort (k_sort_partial), the binned sort (k_sort_binned,
// k_sort_binned_split) and rocPRIM's device-wide sort (k_compose_keys, k_iota; called from bpr_refresh.hip).
// What they must agree on bit for bit — a column's moments, a key's bin, a key's rank inside its bin — is
// defined ONCE, in bpr_sort_shared.h.
#pragma once
#include <rocprim/block/block_radix_sort.hpp>

#include "bpr_ctx.h"
#include "bpr_sort_shared.h"

// bits per pass of the in-LDS block radix sort (0 = rocPRIM's default, 8)
#ifndef BPR_SORT_RADIX_BITS
#define BPR_SORT_RADIX_BITS 0
#endif

namespace bpr {

// Q [I, d] → T [d, I] through a padded 32x32 LDS tile (coalesced on both sides)
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ Q,
                                                   float* __restrict__ T, int64_t I, int d,
                                                   double* __restrict__ sig_acc) {
  __shared__ float tile[32][33];
  // also clears the per-factor sigma accumulators of a split sort (saves a memset launch)
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int k = threadIdx.x; k < 2 * d; k += 256) sig_acc[k] = 0.0;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t i0 = (int64_t)blockIdx.x * 32;
  const int f0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int64_t i = i0 + ty + r;
    const int f = f0 + tx;
    tile[ty + r][tx] = (i < I && f < d) ? Q[i * d + f] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 32; r += 8) {
    const int f = f0 + ty + r;
    const int64_t i = i0 + tx;
    if (f < d && i < I) T[(int64_t)f * I + i] = tile[tx][ty + r];
  }
}

// sigma_f = std(Q[1:, f], unbiased): one block per factor over the contiguous transposed row
__global__ __launch_bounds__(256) void k_sigma(const float* __restrict__ T, int64_t I,
                                               float* __restrict__ sigma) {
  __shared__ double red[256];
  const float* row = T + (int64_t)blockIdx.x * I;
  double s = 0.0;
  for (int64_t i = 1 + threadIdx.x; i < I; i += 256) s += (double)row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double mean = red[0] / (double)(I - 1);
  __syncthreads();
  double ss = 0.0;
  for (int64_t i = 1 + threadIdx.x; i < I; i += 256) {
    const double c = (double)row[i] - mean;
    ss += c * c;
  }
  red[threadIdx.x] = ss;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) sigma[blockIdx.x] = (float)sqrt(red[0] / (double)(I - 2));
}

// ---------------------------------------------------------------------------------------------
// Fast path (I <= 36,864 items): ONE 1024-thread workgroup per factor sorts the whole column in
// registers + LDS (rocprim::block_radix_sort — LSD radix, stable, so ties keep ascending item id) and
// computes sigma_f on the way: d independent workgroups, no inter-block traffic, no memsets.
// The column sits in 1024 x ITEMS registers; the ~100 KiB of LDS is the radix exchange buffer.
// ---------------------------------------------------------------------------------------------
// the block radix sort of k_sort_sub and k_sort_flagged (their load and store loops stay apart: written as one
// helper with callbacks they cost k_sort_sub<36> 20 bytes of scratch more)
template <int ITEMS>
using ColumnSort = rocprim::block_radix_sort<float, 1024, ITEMS, uint16_t, 1, 1, BPR_SORT_RADIX_BITS>;

// Block (s, f) sorts sub-column s of factor f: items [s*len, min((s+1)*len, I)).  With SUB == 1 the
// result is the final order; otherwise sorted (key, id) runs go to scratch for k_merge_runs, so
// that 2 (or 4) workgroups per factor share the work and all 256 CUs are busy.
template <int ITEMS>
__global__ __launch_bounds__(1024) void k_sort_sub(const float* __restrict__ T, int64_t I,
                                                   int64_t len, int32_t* __restrict__ order,
                                                   float* __restrict__ keys_out,
                                                   int32_t* __restrict__ ids_out,
                                                   float* __restrict__ sigma,
                                                   double* __restrict__ sig_acc,
                                                   const int32_t* __restrict__ only_flagged = nullptr) {
  __shared__ union {
    typename ColumnSort<ITEMS>::storage_type sort;
    double red[2][16];
  } sm;
  const int f = blockIdx.y;
  if (only_flagged != nullptr && only_flagged[2 * f] >= 0) return;  // (the fallback of k_sort_binned_split)
  const int64_t base = (int64_t)blockIdx.x * len;
  const int64_t cnt = min(len, I - base);
  const bool single = gridDim.x == 1;
  const float* row = T + (int64_t)f * I;
  const int t = threadIdx.x;
  float keys[ITEMS];
  uint16_t vals[ITEMS];
  ColumnMoments<false> m;
  const float first = row[1];  // shift: removes the mean's magnitude from the sums
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int64_t l = (int64_t)t * ITEMS + k;  // blocked arrangement: sort stability = item order
    const bool valid = l < cnt;
    const float v = valid ? row[base + l] : -__builtin_huge_valf();
    keys[k] = v;
    vals[k] = (uint16_t)l;
    if (valid && base + l >= 1) m.add(v, first);
  }
  m.reduce(t, sm.red);
  if (t == 0) {
    double a, b;
    m.sums(sm.red, &a, &b);
    if (single) {
      sigma[f] = (float)sigma_from_sums(a, b, I);
    } else {  // finalised by k_merge_runs (last level)
      atomicAdd(&sig_acc[2 * f + 0], a);
      atomicAdd(&sig_acc[2 * f + 1], b);
    }
  }
  __syncthreads();
  ColumnSort<ITEMS>().sort_desc_to_striped(keys, vals, sm.sort);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int64_t pos = (int64_t)k * 1024 + t;
    if (pos < cnt) {
      const int64_t o = (int64_t)f * I + base + pos;
      if (single) {
        order[o] = (int32_t)(base + vals[k]);
      } else {
        keys_out[o] = keys[k];
        ids_out[o] = (int32_t)(base + vals[k]);
      }
    }
  }
}

// Merge neighbouring sorted runs of length `run` (descending keys; on equal keys the left run —
// lower item ids — goes first, which keeps the order identical to a stable full sort).
// Two-level merge path.  A workgroup owns MERGE_TILE consecutive outputs of one pair of runs: two
// lanes find where the tile starts and ends in both runs (binary search along the cross diagonals,
// in HBM), the block copies those two slices — at most MERGE_TILE elements together — into LDS with
// coalesced loads, every thread then finds its own MERGE_PER_THREAD outputs by a second diagonal
// search in LDS and merges serially out of LDS; results go back through LDS so the stores are
// coalesced as well.  LDS indices are padded by one word per 16 so the threads' serial walks spread
// over the banks.  HBM traffic: keys + ids read once, written once (ids only on the last level).
#ifndef BPR_MERGE_PER_THREAD
#define BPR_MERGE_PER_THREAD 16
#endif
constexpr int MERGE_PER_THREAD = BPR_MERGE_PER_THREAD;
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_TILE = MERGE_THREADS * MERGE_PER_THREAD;
__device__ __forceinline__ int merge_pad(int k) { return k + k / MERGE_PER_THREAD; }

// number of elements the first `k` merged outputs take from run A (lenA) — B (lenB) gets k - that
template <typename KeyA, typename KeyB>
__device__ __forceinline__ int64_t merge_split(int64_t k, int64_t lenA, int64_t lenB,
                                               const KeyA& A, const KeyB& B) {
  int64_t lo = max((int64_t)0, k - lenB), hi = min(k, lenA);
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A(mid) >= B(k - mid - 1)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MERGE_THREADS) void k_merge_runs(
    const float* __restrict__ keys_in, const int32_t* __restrict__ ids_in, int64_t I, int64_t run,
    int tiles_per_pair, float* __restrict__ keys_out, int32_t* __restrict__ ids_out, int last,
    float* __restrict__ sigma, const double* __restrict__ sig_acc,
    const int32_t* __restrict__ only_flagged = nullptr) {
  __shared__ float lk[MERGE_TILE + MERGE_THREADS + 1];
  __shared__ int32_t lv[MERGE_TILE + MERGE_THREADS + 1];
  __shared__ int64_t cut[2];
  const int f = blockIdx.y;
  const int t = threadIdx.x;
  if (only_flagged != nullptr && only_flagged[2 * f] >= 0) return;
  if (last && blockIdx.x == 0 && t == 0) sigma[f] = (float)sigma_from_sums(sig_acc[2 * f], sig_acc[2 * f + 1], I);
  const int64_t pair = blockIdx.x / tiles_per_pair;
  const int64_t tile = blockIdx.x % tiles_per_pair;
  const int64_t a0 = pair * 2 * run;
  if (a0 >= I) return;
  const int64_t lenA = min(run, I - a0);
  const int64_t b0 = a0 + lenA;
  const int64_t lenB = max((int64_t)0, min(run, I - b0));
  const int64_t k0 = tile * MERGE_TILE;
  if (k0 >= lenA + lenB) return;
  const int64_t k1 = min(k0 + MERGE_TILE, lenA + lenB);
  const float* K = keys_in + (int64_t)f * I;
  const int32_t* V = ids_in + (int64_t)f * I;
  if (t < 128) {
    // 64-ary diagonal search in HBM: wave 0 finds the start of the tile, wave 1 its end.  The
    // predicate "A(x) >= B(k-x-1)" is true on a prefix of [lo, hi); every lane probes one point per
    // step, so the interval shrinks 65-fold per round trip (3 instead of 17 dependent loads).
    const int l = t & 63;
    const int64_t k = t < 64 ? k0 : k1;
    int64_t lo = max((int64_t)0, k - lenB), hi = min(k, lenA);
    while (lo < hi) {
      const int64_t span = hi - lo;
      const bool fine = span <= 64;  // last step: one lane per remaining position
      const int64_t x = fine ? lo + l : lo + (int64_t)(l + 1) * span / 65;
      const bool in = x < hi;
      const bool pred = in && K[a0 + x] >= K[b0 + (k - x - 1)];
      const int c = __popcll(__ballot(pred));  // trues form a prefix of the probes
      if (fine) {
        lo += c;
        hi = lo;
      } else {
        const int64_t below = c == 0 ? lo : lo + (int64_t)c * span / 65 + 1;
        const int64_t above = c == 64 ? hi : lo + (int64_t)(c + 1) * span / 65;
        lo = below;
        hi = above;
      }
    }
    if (l == 0) cut[t >> 6] = lo;
  }
  __syncthreads();
  const int64_t a_lo = cut[0], a_hi = cut[1];
  const int64_t b_lo = k0 - a_lo, b_hi = k1 - a_hi;
  const int nA = (int)(a_hi - a_lo), nB = (int)(b_hi - b_lo);
  for (int x = t; x < nA + nB; x += MERGE_THREADS) {
    const int64_t src = x < nA ? a0 + a_lo + x : b0 + b_lo + (x - nA);
    lk[merge_pad(x)] = K[src];
    lv[merge_pad(x)] = V[src];
  }
  __syncthreads();
  const int n_tile = (int)(k1 - k0);
  const int kk = min(t * MERGE_PER_THREAD, n_tile);
  const int n_out = min(MERGE_PER_THREAD, n_tile - kk);
  int a = (int)merge_split(kk, nA, nB, [&](int64_t x) { return lk[merge_pad((int)x)]; },
                           [&](int64_t x) { return lk[merge_pad(nA + (int)x)]; });
  int b = kk - a;
  float ok[MERGE_PER_THREAD];
  int32_t ov[MERGE_PER_THREAD];
  float ka = a < nA ? lk[merge_pad(a)] : 0.f, kb = b < nB ? lk[merge_pad(nA + b)] : 0.f;
#pragma unroll
  for (int q = 0; q < MERGE_PER_THREAD; ++q) {
    const bool take_a = (a < nA) && (b >= nB || ka >= kb);
    if (q < n_out) {
      ov[q] = lv[merge_pad(take_a ? a : nA + b)];
      ok[q] = take_a ? ka : kb;
      if (take_a) {
        ++a;
        ka = a < nA ? lk[merge_pad(a)] : 0.f;
      } else {
        ++b;
        kb = b < nB ? lk[merge_pad(nA + b)] : 0.f;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < MERGE_PER_THREAD; ++q) {
    if (q < n_out) {
      lk[merge_pad(kk + q)] = ok[q];
      lv[merge_pad(kk + q)] = ov[q];
    }
  }
  __syncthreads();
  const int64_t o_base = (int64_t)f * I + a0 + k0;
  for (int x = t; x < n_tile; x += MERGE_THREADS) {
    ids_out[o_base + x] = lv[merge_pad(x)];
    if (!last) keys_out[o_base + x] = lk[merge_pad(x)];
  }
}

// ---------------------------------------------------------------------------------------------
// PARTIAL snapshot (r5): what the adaptive sampler reads of a column is its two ends
// — rank Geometric(p) + seen-skips from the top or from the bottom (neg_samplers.py:90-121) — so only
// the ends are sorted exactly and the middle is BUCKETED:
//   order[0 .. Kt)        the Kt largest keys, exact descending order (ties by ascending id)
//   order[Kt .. I - Kb)   the middle in MID_BINS value-linear bins, bins in descending key order,
//                         any order inside a bin; the first entry of a bin carries MID_FLAG
//   order[I - Kb .. I)    the Kb smallest keys, exact (the first of them carries MID_FLAG too)
// Kt / Kb come from two cuts read off a coarse histogram of the column (any counts are legal;
// meta[f] = {Kt, Kb}).  A walk that leaves an exact end keeps counting unseen entries — counting
// does not care about the order inside a bin — and finishes INSIDE one bin by ranking its <= MID_BIN_MAX
// keys on the fly (bpr_device.h adaptive_finish_in_bin).  A column the scheme does not fit (a threshold
// that does not separate, an end that overflows its compaction buffer, a bin with more than
// MID_BIN_MAX keys: many equal keys) reports meta[f] = {-1, -1} and is sorted whole by the kernel
// launched behind this one (k_sort_sub over the flagged columns).
// One 1024-thread workgroup per column, I <= 1024 * ITEMS.
// ---------------------------------------------------------------------------------------------
constexpr int MID_BINS = 4096;
constexpr int MID_BIN_MAX = 64;
constexpr int PART_CI = 2;                    // compacted keys per thread in the sort of the two ends
constexpr int PART_CAP = 1024 * PART_CI / 2;  // ... i.e. at most 1,024 keys per end
constexpr uint32_t MID_FLAG = 0x80000000u;    // == bpr::ORDER_FLAG (bpr_device.h)

template <int ITEMS>
__global__ __launch_bounds__(1024) void k_sort_partial(const float* __restrict__ T, int64_t I,
                                                       int32_t* __restrict__ order,
                                                       float* __restrict__ sigma,
                                                       int32_t* __restrict__ meta, int target) {
  using EndSort = rocprim::block_radix_sort<float, 1024, PART_CI, uint16_t>;
  __shared__ union {
    typename EndSort::storage_type ends;
    double red[2][16];
  } sm;
  __shared__ float s_ck[2 * PART_CAP];     // compacted keys: [0, CAP) the top end, [CAP, 2 CAP) the bottom end
  __shared__ uint16_t s_ci[2 * PART_CAP];  // ... and their item ids
  __shared__ uint32_t s_hist[MID_BINS];    // keys per middle bin, then the bins' first positions
  __shared__ uint32_t s_coarse[1024];      // keys per coarse bin of the whole column
  __shared__ uint32_t s_cum[1024];         // ... and before it, from the top
  __shared__ uint32_t s_scan[1024];
  __shared__ int32_t s_cnt[4];             // the cuts' coarse bins, largest middle bin
  __shared__ int32_t s_mid[1024 * ITEMS];  // the middle, staged: written back in whole lines (a scattered 4-byte
                                           // store is a 64-B write request at the memory side — the very
                                           // resource k_stream, running beside this kernel, is bound by)
  const int f = blockIdx.x;
  const float* row = T + (int64_t)f * I;
  const int t = threadIdx.x;
  const int n = (int)I;
  float keys[ITEMS];
  ColumnMoments<false> m;
  const float first = row[1];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int l = t * ITEMS + k;  // blocked: a thread's ids ascend, and so do the threads'
    const bool valid = l < n;
    const float v = valid ? row[l] : 0.f;
    keys[k] = v;
    if (valid && l >= 1) m.add(v, first);
  }
  for (int k = t; k < MID_BINS; k += 1024) s_hist[k] = 0u;
  s_coarse[t] = 0u;
  if (t < 4) s_cnt[t] = t == 1 ? 1023 : 0;  // [0] / [1]: the cuts' coarse bins (defaults: nothing in the ends)
  m.reduce(t, sm.red);
  if (t == 0) {
    double a, b;
    m.sums(sm.red, &a, &b);
    sigma[f] = (float)sigma_from_sums(a, b, I);
    sm.red[0][0] = a;  // the totals, for everybody (the coarse bins' range)
    sm.red[1][0] = b;
  }
  __syncthreads();
  // ---- a coarse histogram of the whole column: 1,024 value-linear bins over mean +- 5 sigma (out-of-range
  // keys in the end bins).  Everything below is decided by a key's coarse bin and its place inside it — a
  // monotone function of the key — so classes and bins agree with the order whatever the rounding, equal keys
  // stay together, and any distribution works: a skewed column gets unequal ends, a column with a spike
  // (the cold items of a trained model: thousands of keys within +-0.004 of zero) gets as many fine bins
  // there as it has keys there (the fine bins are cut along the coarse CDF, not along the value axis).
  float cmax, cscale;
  {
    const double a = sm.red[0][0], b = sm.red[1][0];
    const double mean = (double)first + a / (double)(I - 1);
    const double sd = sigma_from_sums(a, b, I);
    cmax = (float)(mean + 5.0 * sd);
    cscale = sd > 0.0 ? (float)(1024.0 / (10.0 * sd)) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (t * ITEMS + k < n) atomicAdd(&s_coarse[coarse_bin(keys[k], cmax, cscale)], 1u);
  __syncthreads();
  s_cum[t] = (uint32_t)block_excl((int)s_coarse[t], t, s_scan);  // keys above coarse bin t
  __syncthreads();
  // ---- classify by a key's interpolated RANK r = (keys above its coarse bin) + (its place inside the bin) x
  // (keys in the bin): top r < target, bottom r >= n - target, middle between; the middle's fine bin is r
  // scaled to MID_BINS.  r is a monotone function of the key (equal keys: equal r), so classes and bins
  // agree with the order; inside a coarse bin the density is taken as uniform, which is what makes the
  // cuts and the bins equi-DEPTH rather than equi-width.
  const float rt = (float)min(target, n / 4), rb = (float)n - rt;
  const bool separates = cscale > 0.f;
  const float fscale = (float)MID_BINS / fmaxf(rb - rt, 1.f);
  int my_top = 0, my_bot = 0;
  uint32_t packed[ITEMS];  // bit 31: not a middle key (bit 0: top); else bin << 8 | ordinal inside the bin
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int l = t * ITEMS + k;
    packed[k] = 0x80000000u;
    if (l >= n || !separates) continue;
    const float x = (cmax - keys[k]) * cscale;
    const int cb = min(1023, max(0, (int)x));
    const float frac = fminf(fmaxf(x - (float)cb, 0.f), 0.999f);
    const float r = (float)s_cum[cb] + frac * (float)s_coarse[cb];
    if (r < rt) {
      packed[k] = 0x80000001u;
      ++my_top;
    } else if (r >= rb) {
      ++my_bot;
    } else {
      const int bin = min(MID_BINS - 1, max(0, (int)((r - rt) * fscale)));
      const uint32_t ord = atomicAdd(&s_hist[bin], 1u);
      packed[k] = ((uint32_t)bin << 8) | min(ord, 255u);
    }
  }
  // ---- the ends' keys in the compaction buffers: block-wide exclusive scans of the threads' counts
  int Kt = 0, Kb = 0, n_mid = 0;
  const int top_at = block_excl_total(my_top, t, s_scan, &Kt);
  const int bot_at = block_excl_total(my_bot, t, s_scan, &Kb);
  n_mid = n - Kt - Kb;
  // ---- the fine bins' sizes -> first positions (exclusive scan over MID_BINS = 4 per thread)
  bins_to_positions<MID_BINS / 1024>(s_hist, t, s_scan, MID_BIN_MAX, &s_cnt[2], [](int, uint32_t) {});
  __syncthreads();
  const bool ok = separates && Kt <= PART_CAP && Kb <= PART_CAP && Kt >= 1 && Kb >= 1 && n_mid >= 0 && s_cnt[2] == 0;
  if (!ok) {  // (uniform over the block) the column is sorted whole by the kernel behind this one
    if (t == 0) {
      meta[2 * f] = -1;
      meta[2 * f + 1] = -1;
    }
    return;
  }
  if (t == 0) {
    meta[2 * f] = Kt;
    meta[2 * f + 1] = Kb;
  }
  // ---- scatter (all in LDS): ends to the compaction buffers (ids ascending among equal keys: the sort is
  // stable), middle keys to their place in the staged middle
  // a key between the two ends for the pads: the smallest top key and the largest bottom key bracket it
  // (block minimum / maximum through s_scan)
  float tmin = __builtin_huge_valf(), bmax = -__builtin_huge_valf();
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    if (t * ITEMS + k >= n || (packed[k] & 0x80000000u) == 0u) continue;
    if (packed[k] & 1u) tmin = fminf(tmin, keys[k]); else bmax = fmaxf(bmax, keys[k]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    tmin = fminf(tmin, __shfl_xor(tmin, off, 64));
    bmax = fmaxf(bmax, __shfl_xor(bmax, off, 64));
  }
  __syncthreads();
  if ((t & 63) == 0) {
    s_scan[t >> 6] = __float_as_uint(tmin);
    s_scan[16 + (t >> 6)] = __float_as_uint(bmax);
  }
  __syncthreads();
  for (int w = 0; w < 16; ++w) {
    tmin = fminf(tmin, __uint_as_float(s_scan[w]));
    bmax = fmaxf(bmax, __uint_as_float(s_scan[16 + w]));
  }
  const float pad_key = 0.5f * tmin + 0.5f * bmax;
  __syncthreads();
  for (int k = t; k < 2 * PART_CAP; k += 1024) {
    // pads sort between the two ends: a key of the middle's range; should it tie with an end's key the pads
    // still sit on the right side of the tie — top keys precede them in the buffer, bottom keys follow them
    s_ck[k] = pad_key;
    s_ci[k] = 0;
  }
  __syncthreads();
  {
    int ta = top_at, ba = bot_at;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int l = t * ITEMS + k;
      if (l >= n) continue;
      if ((packed[k] & 0x80000000u) == 0u) {
        const int bin = (int)(packed[k] >> 8), ord = (int)(packed[k] & 255u);
        s_mid[(int)s_hist[bin] + ord] = (int32_t)((uint32_t)l | (ord == 0 ? MID_FLAG : 0u));
      } else if (packed[k] & 1u) {
        s_ck[ta] = keys[k];
        s_ci[ta] = (uint16_t)l;
        ++ta;
      } else {
        // the bottom end sits at the END of its half: pads before it, so that pads win ties with it
        const int at = 2 * PART_CAP - Kb + ba;
        s_ck[at] = keys[k];
        s_ci[at] = (uint16_t)l;
        ++ba;
      }
    }
  }
  __syncthreads();
  int32_t* col = order + (int64_t)f * I;
  for (int k = t; k < n_mid; k += 1024) col[Kt + k] = s_mid[k];  // whole lines
  // ---- the two ends in ONE stable descending sort of 2 x PART_CAP (key, id) pairs
  float ek[PART_CI];
  uint16_t ev[PART_CI];
#pragma unroll
  for (int k = 0; k < PART_CI; ++k) {
    ek[k] = s_ck[t * PART_CI + k];
    ev[k] = s_ci[t * PART_CI + k];
  }
  __syncthreads();
  EndSort().sort_desc_to_striped(ek, ev, sm.ends);
#pragma unroll
  for (int k = 0; k < PART_CI; ++k) {
    const int pos = k * 1024 + t;  // rank in the sorted sequence: top end, pads, bottom end
    if (pos < Kt) col[pos] = (int32_t)ev[k];
    else if (pos >= 2 * PART_CAP - Kb) {
      const int b = pos - (2 * PART_CAP - Kb);  // 0 .. Kb-1
      col[n - Kb + b] = (int32_t)((uint32_t)ev[k] | (b == 0 ? MID_FLAG : 0u));
    }
  }
}

// the columns k_sort_partial gave up on (meta[f] < 0), sorted whole: k_sort_sub's single-workgroup form
template <int ITEMS>
__global__ __launch_bounds__(1024) void k_sort_flagged(const float* __restrict__ T, int64_t I,
                                                       int32_t* __restrict__ order,
                                                       int32_t* __restrict__ meta) {
  __shared__ typename ColumnSort<ITEMS>::storage_type sm;
  const int f = blockIdx.x;
  if (meta[2 * f] >= 0) return;
  const float* row = T + (int64_t)f * I;
  const int t = threadIdx.x;
  float keys[ITEMS];
  uint16_t vals[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int64_t l = (int64_t)t * ITEMS + k;
    keys[k] = l < I ? row[l] : -__builtin_huge_valf();
    vals[k] = (uint16_t)l;
  }
  ColumnSort<ITEMS>().sort_desc_to_striped(keys, vals, sm);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int64_t pos = (int64_t)k * 1024 + t;
    if (pos < I) order[(int64_t)f * I + pos] = (int32_t)vals[k];
  }
  __syncthreads();
  if (t == 0) {
    meta[2 * f] = (int32_t)I;  // every position exact
    meta[2 * f + 1] = 0;
  }
}

// ---------------------------------------------------------------------------------------------
// BINNED snapshot sort (r5): the WHOLE column in exact descending order (ties by
// ascending item id, -0 == +0: the order of the stable radix sort above, bit for bit) without a radix sort.
// An interpolated rank — a monotone function of the key read off a 1,024-bin histogram of the column's
// [min, max] and a second 1,024-bin level over its crowded stretch — drops every key into one of BINS equi-DEPTH bins (n / BINS ~ 2.5 keys each);
// a one-pass counting sort stages (orderable key, id) by bin in LDS; then, POSITION by position (a
// wave takes 64 consecutive staged entries: its lanes read the same few words — broadcasts, no bank
// conflicts — and find their bin's bounds from three ballots of first-of-bin flags), every key counts
// the members of its bin that precede it; the ids move to their final places in LDS and leave in
// whole lines.  Work per key: two LDS atomics, two LDS writes, ~bin-size LDS reads — against eight
// (radix 4) or four (radix 8) ranked LDS exchanges of the 32-bit radix sort.  A column the scheme does
// not fit (a bin over BIN_MAX keys: a spike narrower than a coarse bin, thousands of equal keys; no
// spread at all) reports meta[2f] = -1 and is sorted whole by k_sort_flagged behind this kernel.
// One 1024-thread workgroup per column, I <= 1024 * ITEMS <= 32,768 (the id shares 16 bits with the
// first-of-bin flag); LDS = 6 B per key + 4 B per bin.
// ---------------------------------------------------------------------------------------------
template <int ITEMS>
__global__ __launch_bounds__(1024) void k_sort_binned(const float* __restrict__ T, int64_t I,
                                                      int32_t* __restrict__ order,
                                                      float* __restrict__ sigma,
                                                      int32_t* __restrict__ meta) {
  static_assert(1024 * ITEMS <= 32768 && ITEMS >= 4, "ids share 16 bits with the first-of-bin flag");
  constexpr int BINS = ITEMS <= 6 ? 2048 : ITEMS <= 10 ? 4096 : 8192;
  constexpr int BPT = BINS / 1024;
  __shared__ uint32_t s_key[1024 * ITEMS + 4];  // orderable keys, staged by bin (before that: the histograms)
  __shared__ uint16_t s_id[1024 * ITEMS];   // their item ids | BIN_FIRST; then the ids in final order
  __shared__ uint32_t s_hist[BINS + 1];     // keys per bin, then the bins' first positions ([BINS]: the pads' bin)
  __shared__ uint32_t s_scan[16];
  __shared__ double s_red[2][16];
  __shared__ float s_mm[2][16];
  __shared__ int32_t s_big;
  __shared__ int32_t s_hull[2];             // the crowded stretch: first / last coarse bin over BIN_CROWD keys
  BinHistogram h;
  h.coarse = s_key;
  h.cum = s_key + 1024;
  h.fine = s_key + 2048;
  h.fcum = s_key + 3072;
  const int f = blockIdx.x;
  const float* row = T + (int64_t)f * I;
  const int t = threadIdx.x;
  const int n = (int)I;
  // (array elements are assigned outside any branch: a conditional store into a register array makes the
  // compiler carry the whole array through the branch as one vector value — 5,600 spilled VGPRs at ITEMS = 20)
  float keys[ITEMS];
  ColumnMoments<true> m;
  const float first = row[1];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int l = k * 1024 + t;  // striped: coalesced loads (the order below does not lean on the arrangement)
    const bool valid = l < n;
    const float v = valid ? row[l] : 0.f;
    keys[k] = v;
    m.add(v, first, valid && l >= 1);
    m.minmax(v, valid);
  }
  for (int k = t; k <= BINS; k += 1024) s_hist[k] = 0u;
  h.coarse[t] = 0u;
  h.fine[t] = 0u;
  if (t == 0) {
    s_big = 0;
    s_hull[0] = 1024;
    s_hull[1] = -1;
  }
  m.reduce(t, s_red, s_mm);
  if (t == 0) {
    double a, b;
    m.sums(s_red, &a, &b);
    sigma[f] = (float)sigma_from_sums(a, b, I);
  }
  // ---- coarse histogram: 1,024 value-linear bins
  m.fold_minmax(s_mm);
  h.set_range(m.vmin, m.vmax);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (k * 1024 + t < n) h.count_coarse(keys[k]);
  __syncthreads();
  h.cum[t] = (uint32_t)block_excl((int)h.coarse[t], t, s_scan);  // keys above coarse bin t
  // ---- second level over the crowded stretch
  h.find_hull(t, s_hull);
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) h.count_fine(keys[k], k * 1024 + t < n);
  __syncthreads();
  h.fcum[t] = (uint32_t)block_excl((int)h.fine[t], t, s_scan);
  __syncthreads();
  h.set_hull_above();
  // ---- a key's bin from its interpolated rank
  const float bscale = (float)BINS / (float)n;
  uint32_t packed[ITEMS];  // bin << 8 | ordinal inside the bin
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int b = h.bin_of(keys[k], BINS, bscale);
    const int bin = k * 1024 + t < n ? b : BINS;
    const uint32_t ord = atomicAdd(&s_hist[bin], 1u);
    packed[k] = ((uint32_t)bin << 8) | min(ord, 255u);
  }
  __syncthreads();
  // ---- the bins' sizes -> first positions
  bins_to_positions<BPT>(s_hist, t, s_scan, BIN_MAX, &s_big, [](int, uint32_t) {});
  __syncthreads();  // (the coarse histogram is dead from here: the staged keys take its place)
  if (s_big != 0 || h.cscale <= 0.f) {  // (uniform over the block) sorted whole by k_sort_flagged
    if (t == 0) {
      meta[2 * f] = -1;
      meta[2 * f + 1] = -1;
    }
    return;
  }
  if (t == 0) {
    meta[2 * f] = n;
    meta[2 * f + 1] = 0;
  }
  // ---- counting sort into LDS; the first entry of a bin carries BIN_FIRST
  if (t < 4) s_key[n + t] = 0u;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const int l = k * 1024 + t;
    const uint32_t ord = packed[k] & 255u;
    const int at = (int)s_hist[packed[k] >> 8] + (int)ord;
    if (l < n) {
      s_key[at] = orderable_desc(keys[k]);
      s_id[at] = (uint16_t)((uint32_t)l | (ord == 0u ? BIN_FIRST : 0u));
    }
  }
  __syncthreads();
  // ---- a key's place inside its bin, position by position (rank_in_window).  A wave walks ITEMS consecutive
  // 64-entry windows; each window's flags — ballots over the ids' BIN_FIRST bits — are read once and handed on.
  const int lane = t & 63;
  uint32_t out[ITEMS];  // final position << 16 | id
  {
    int base = (t >> 6) * ITEMS * 64;
    uint32_t me = base + lane < n ? (uint32_t)s_id[base + lane] : 0u;
    const uint32_t before = base >= 64 && base + lane - 64 < n ? (uint32_t)s_id[base + lane - 64] : 0u;
    unsigned long long bc = __ballot((me & BIN_FIRST) != 0u || base + lane == n);
    unsigned long long bp = __ballot((before & BIN_FIRST) != 0u);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int p = base + lane;
      const uint32_t next = p + 64 < n ? (uint32_t)s_id[p + 64] : 0u;
      const unsigned long long bn = __ballot((next & BIN_FIRST) != 0u || p + 64 == n);
      const int id = (int)(me & (BIN_FIRST - 1u));
      const int pos = rank_in_window(s_key, base, lane, n, bp, bc, bn, id,
                                     [&](int j) { return (int)((uint32_t)s_id[j] & (BIN_FIRST - 1u)); });
      out[k] = ((uint32_t)pos << 16) | (uint32_t)id;
      bp = bc;
      bc = bn;
      me = next;
      base += 64;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (((t >> 6) * ITEMS + k) * 64 + lane < n) s_id[out[k] >> 16] = (uint16_t)(out[k] & 0xffffu);
  __syncthreads();
  int32_t* col = order + (int64_t)f * I;
  for (int k = t; k < n; k += 1024) col[k] = (int32_t)s_id[k];  // whole lines
}

// ---------------------------------------------------------------------------------------------
// The binned sort with G workgroups per column: workgroup g orders the g-th stretch of RANKS.  For columns
// that do not fit one workgroup's LDS (20,480 < I <= 131,071: MSD's 41,141, Yelp's 92,090).  Every workgroup reads
// the whole column
// (L2-resident) and builds the same two-level histogram; nothing is kept in registers between passes — a
// count pass and a fill pass over the keys replace the remembered ordinals — and only the keys whose bin falls
// into its stretch are staged: about I / G, at most 1,024 x SITEMS.  The first-of-bin flags live in a bit
// array (past 32,767 items the ids need all 16 bits): a 64-entry window's flags are one 64-bit word.  Its part
// of the order starts at (keys above its stretch).  A workgroup that cannot (a bin over BIN_MAX keys, a
// stretch over its capacity, no spread) flags the column — meta[2f] = -1, cleared to 0 before the launch — and
// the radix path behind it redoes exactly the flagged columns.
// WIDE (k_sort_binned_split<SPLIT_WIDE + SITEMS>, 65,536 <= I <= 131,071): the 17th bit of an id lives in a bit array beside the
// 16-bit ids, one bit per staged entry — 2.5 KB at CAP = 20,480, so the staged stretch stays as long as with 16-bit
// ids and G as small (32-bit ids would fit 12,288 entries at most: G = 8 instead of 5 for 92,090 items, and every
// workgroup repeats the five passes over the column).  A window's high bits are one 64-bit word, as its flags are;
// the ids in final order take theirs from s_hist's first words, which the fill pass leaves dead.
// ---------------------------------------------------------------------------------------------
constexpr int SPLIT_BINS = 4096;  // bins per workgroup

template <int CAP>
__device__ __forceinline__ uint32_t* split_high_bits() {  // (only a WIDE instantiation owns the array)
  __shared__ uint32_t s_hi[CAP / 32];
  return s_hi;
}

// SITEMS_W = SITEMS, or SPLIT_WIDE + SITEMS for the WIDE form (one kernel template, and the 16-bit instantiations
// keep their symbols and their code)
constexpr int SPLIT_WIDE = 64;

template <int SITEMS_W>
__global__ __launch_bounds__(1024) void k_sort_binned_split(const float* __restrict__ T, int64_t I,
                                                            int32_t* __restrict__ order,
                                                            float* __restrict__ sigma,
                                                            int32_t* __restrict__ meta) {
  constexpr bool WIDE = SITEMS_W >= SPLIT_WIDE;
  constexpr int SITEMS = WIDE ? SITEMS_W - SPLIT_WIDE : SITEMS_W;
  constexpr int CAP = 1024 * SITEMS;
  constexpr int BPT = SPLIT_BINS / 1024;
  static_assert(CAP / 32 <= SPLIT_BINS, "the final order's high id bits live in s_hist");
  __shared__ uint32_t s_key[CAP + 4];
  __shared__ uint16_t s_id[CAP];             // the ids' low 16 bits
  __shared__ uint32_t s_flag[CAP / 32 + 4];  // first-of-bin bits
  uint32_t* s_hi = nullptr;                  // bit 16 of the staged ids
  if constexpr (WIDE) s_hi = split_high_bits<CAP>();
  __shared__ uint32_t s_hist[SPLIT_BINS];
  __shared__ uint32_t s_coarse[1024], s_cum[1024], s_fine[1024], s_fcum[1024];
  __shared__ uint32_t s_scan[16];
  __shared__ double s_red[2][16];
  __shared__ float s_mm[2][16];
  __shared__ int32_t s_big;
  __shared__ int32_t s_hull[2];
  __shared__ int32_t s_tot[2];
  BinHistogram h;
  h.coarse = s_coarse;
  h.cum = s_cum;
  h.fine = s_fine;
  h.fcum = s_fcum;
  const int g = blockIdx.x, G = gridDim.x;
  const int f = blockIdx.y;
  const float* row = T + (int64_t)f * I;
  const int t = threadIdx.x;
  const int n = (int)I;
  const int items = (n + 1023) / 1024;
  // a pass over the column: eight loads in flight, then the work on them (a load per trip would leave every
  // trip waiting for the L2: 5 passes x 41 trips x ~0.6 us on MSD)
  auto for_keys = [&](auto&& fn) {
    for (int k0 = 0; k0 < items; k0 += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int l = (k0 + q) * 1024 + t;
        v[q] = l < n ? row[l] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int l = (k0 + q) * 1024 + t;
        if (l < n) fn(l, v[q]);
      }
    }
  };
  // ---- pass 1: sigma, min, max (the sums in k_sort_binned's order)
  ColumnMoments<true> m;
  const float first = row[1];
  for_keys([&](int l, float v) {
    if (l >= 1) m.add(v, first);
    m.minmax(v);
  });
  for (int k = t; k < SPLIT_BINS; k += 1024) s_hist[k] = 0u;
  for (int k = t; k < CAP / 32 + 4; k += 1024) s_flag[k] = 0u;
  if constexpr (WIDE)
    for (int k = t; k < CAP / 32; k += 1024) s_hi[k] = 0u;
  s_coarse[t] = 0u;
  s_fine[t] = 0u;
  if (t == 0) {
    s_big = 0;
    s_hull[0] = 1024;
    s_hull[1] = -1;
  }
  m.reduce(t, s_red, s_mm);
  if (t == 0 && g == 0) {
    double a, b;
    m.sums(s_red, &a, &b);
    sigma[f] = (float)sigma_from_sums(a, b, I);
  }
  m.fold_minmax(s_mm);
  h.set_range(m.vmin, m.vmax);
  // ---- pass 2: the coarse histogram
  for_keys([&](int, float v) { h.count_coarse(v); });
  __syncthreads();
  s_cum[t] = (uint32_t)block_excl((int)s_coarse[t], t, s_scan);
  h.find_hull(t, s_hull);
  // ---- pass 3: the second level over the crowded stretch
  for_keys([&](int, float v) { h.count_fine(v); });
  __syncthreads();
  s_fcum[t] = (uint32_t)block_excl((int)s_fine[t], t, s_scan);
  __syncthreads();
  h.set_hull_above();
  const int all_bins = G * SPLIT_BINS;  // the key's bin among all G x SPLIT_BINS
  const float bscale = (float)all_bins / (float)n;
  const int my_lo = g * SPLIT_BINS;
  // ---- pass 4: this stretch's bins counted, and the keys above the stretch
  int above = 0;
  for_keys([&](int, float v) {
    const int b = h.bin_of(v, all_bins, bscale) - my_lo;
    above += b < 0 ? 1 : 0;
    if (b >= 0 && b < SPLIT_BINS) atomicAdd(&s_hist[b], 1u);
  });
  __syncthreads();
  {
    const int before = block_excl(above, t, s_scan);
    if (t == 1023) s_tot[0] = before + above;
    // (a bin's first position: the fill pass counts it up)
    const int end = bins_to_positions<BPT>(s_hist, t, s_scan, BIN_MAX, &s_big, [&](int at, uint32_t size) {
      if (size != 0u && at < CAP) atomicOr(&s_flag[at >> 5], 1u << (at & 31));
    });
    if (t == 1023) s_tot[1] = end;
  }
  __syncthreads();
  const int rank0 = s_tot[0], n_mine = s_tot[1];
  if (s_big != 0 || h.cscale <= 0.f || n_mine > CAP) {  // (uniform over the block)
    if (t == 0) meta[2 * f] = -1;
    return;
  }
  if (t == 0) atomicOr(&s_flag[n_mine >> 5], 1u << (n_mine & 31));  // the end counts as a bin's first entry
  if (t < 4) s_key[n_mine + t] = 0u;                                 // ... and past it the smallest orderable key
  // ---- pass 5: fill
  for_keys([&](int l, float v) {
    const int b = h.bin_of(v, all_bins, bscale) - my_lo;
    if (b >= 0 && b < SPLIT_BINS) {
      const int at = (int)atomicAdd(&s_hist[b], 1u);
      s_key[at] = orderable_desc(v);
      s_id[at] = (uint16_t)l;
      if constexpr (WIDE)
        if (l >> 16) atomicOr(&s_hi[at >> 5], 1u << (at & 31));
    }
  });
  __syncthreads();
  if constexpr (WIDE)  // (the bins' cursors are dead: the high id bits of the final order; the barrier behind the
    for (int k = t; k < CAP / 32; k += 1024) s_hist[k] = 0u;  // ranking orders this before the scatter)
  // ---- ranking inside the bins, position by position (rank_in_window; a window's flags are one 64-bit word)
  const int lane = t & 63;
  uint32_t out[SITEMS];  // final position << 16 | id ... two words past 32,767 items: position and id apart
  uint32_t oid[SITEMS];
  {
    int base = (t >> 6) * SITEMS * 64;
#pragma unroll
    for (int k = 0; k < SITEMS; ++k) {
      const int p = base + lane;
      const bool valid = p < n_mine;
      const int w = base >> 5;  // (base is a multiple of 64)
      const unsigned long long bc = (unsigned long long)s_flag[w] | ((unsigned long long)s_flag[w + 1] << 32);
      const unsigned long long bp = base >= 64 ? (unsigned long long)s_flag[w - 2] | ((unsigned long long)s_flag[w - 1] << 32) : 0ull;
      const unsigned long long bn = base + 64 <= CAP ? (unsigned long long)s_flag[w + 2] | ((unsigned long long)s_flag[w + 3] << 32) : 0ull;
      int id = valid ? (int)s_id[p] : 0;
      if constexpr (WIDE) {
        const unsigned long long bh = (unsigned long long)s_hi[w] | ((unsigned long long)s_hi[w + 1] << 32);
        id |= valid ? (int)((bh >> lane) & 1ull) << 16 : 0;
      }
      out[k] = (uint32_t)rank_in_window(s_key, base, lane, n_mine, bp, bc, bn, id, [&](int j) {
        if constexpr (WIDE) return (int)s_id[j] | (int)((s_hi[j >> 5] >> (j & 31)) & 1u) << 16;
        else return (int)s_id[j];
      });
      oid[k] = (uint32_t)id;
      base += 64;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SITEMS; ++k)
    if (((t >> 6) * SITEMS + k) * 64 + lane < n_mine) {
      s_id[out[k]] = (uint16_t)oid[k];
      if constexpr (WIDE)
        if (oid[k] >> 16) atomicOr(&s_hist[out[k] >> 5], 1u << (out[k] & 31));
    }
  __syncthreads();
  int32_t* col = order + (int64_t)f * I + rank0;
  if constexpr (WIDE) {
    for (int k = t; k < n_mine; k += 1024)
      col[k] = (int32_t)((uint32_t)s_id[k] | ((s_hist[k >> 5] >> (k & 31)) & 1u) << 16);
  } else {
    for (int k = t; k < n_mine; k += 1024) col[k] = (int32_t)s_id[k];
  }
}

// composite sort key: (factor << 32) | ~orderable(value)  → ascending sort = per-factor descending
__global__ void k_compose_keys(const float* __restrict__ T, uint64_t* __restrict__ keys, int64_t n,
                               int64_t I) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    uint32_t b = __float_as_uint(T[k]);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    keys[k] = ((uint64_t)(k / I) << 32) | (uint64_t)(~b);
  }
}

__global__ void k_iota(int32_t* ids, int32_t* offs, int64_t I, int d) {
  const int64_t n = (int64_t)d * I;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x)
    ids[k] = (int32_t)(k % I);
  if (blockIdx.x == 0)
    for (int f = threadIdx.x; f <= d; f += blockDim.x) offs[f] = (int32_t)((int64_t)f * I);
}

}  // namespace bpr
