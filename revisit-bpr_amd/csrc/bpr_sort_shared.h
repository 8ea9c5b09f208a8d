// bpr_sort_shared.h — what the snapshot's sort kernels (bpr_sort.h) have in common: a column's moments and sigma,
// the block-wide scan, the binned sorters' histogram with the bin it gives a key, and the rank of a key inside
// its bin.  Each piece is defined once so that the sorters agree bit for bit.  Plain HIP, no rocPRIM
// (tools/ubench/make_binned_bench.py compiles this header with k_sort_binned alone).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpr {

// ---------------------------------------------------------------------------------------------
// Shared pieces of the sorters (1,024-thread workgroups, 16 waves)
// ---------------------------------------------------------------------------------------------
constexpr int BIN_MAX = 64;  // (the ballots of the binned sort look one 64-entry window back and one ahead)
constexpr int BIN_CROWD = 32;
constexpr uint32_t BIN_FIRST = 0x8000u;

__device__ __forceinline__ uint32_t orderable_desc(float v) {  // larger float <=> larger uint; -0 == +0, as a
  uint32_t b = __float_as_uint(v);                             // comparison and rocPRIM's radix digits have it
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// sigma_f = unbiased std over rows 1..I-1 (neg_samplers.py:132) from the shifted sums a = sum(v - first),
// b = sum((v - first)^2)
__device__ __forceinline__ double sigma_from_sums(double a, double b, int64_t I) {
  const double n = (double)(I - 1);
  return sqrt(fmax(b - a * a / n, 0.0) / (n - 1.0));
}

// A column's moments: every thread adds its keys (in the order its kernel loads them: the sum order is the
// kernel's), reduce() leaves 16 per-wave partials in LDS, which thread 0 sums (sums) and every thread
// folds (minmax).  `first` (row 1's key) is the shift that removes the mean's magnitude from the sums.
template <bool MINMAX>
struct ColumnMoments {
  double s1 = 0.0, s2 = 0.0;
  float vmin = __builtin_huge_valf(), vmax = -__builtin_huge_valf();
  __device__ __forceinline__ void add(float v, float first, bool on = true) {
    const double c = (double)v - (double)first;
    s1 += on ? c : 0.0;
    s2 += on ? c * c : 0.0;
  }
  __device__ __forceinline__ void minmax(float v, bool on = true) {
    vmin = on ? fminf(vmin, v) : vmin;
    vmax = on ? fmaxf(vmax, v) : vmax;
  }
  __device__ __forceinline__ void reduce(int t, double (*red)[16], float (*mm)[16] = nullptr) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
      if constexpr (MINMAX) {
        vmin = fminf(vmin, __shfl_xor(vmin, off, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
      }
    }
    if ((t & 63) == 0) {
      red[0][t >> 6] = s1;
      red[1][t >> 6] = s2;
      if constexpr (MINMAX) {
        mm[0][t >> 6] = vmin;
        mm[1][t >> 6] = vmax;
      }
    }
    __syncthreads();
  }
  static __device__ __forceinline__ void sums(const double (*red)[16], double* a, double* b) {
    double x = 0.0, y = 0.0;
    for (int w = 0; w < 16; ++w) {
      x += red[0][w];
      y += red[1][w];
    }
    *a = x;
    *b = y;
  }
  __device__ __forceinline__ void fold_minmax(const float (*mm)[16]) {
    for (int w = 0; w < 16; ++w) {
      vmin = fminf(vmin, mm[0][w]);
      vmax = fmaxf(vmax, mm[1][w]);
    }
  }
};

// Exclusive prefix of one value per thread over the block (s_scan: 16 words).  block_excl_total also hands
// everybody the block's sum.
__device__ __forceinline__ int wave_incl_scan(int v, int t) {
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(incl, off, 64);
    if ((t & 63) >= off) incl += u;
  }
  return incl;
}
__device__ __forceinline__ int block_excl(int v, int t, uint32_t* s_scan) {
  const int incl = wave_incl_scan(v, t);
  __syncthreads();
  if ((t & 63) == 63) s_scan[t >> 6] = (uint32_t)incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < (t >> 6); ++w) base += (int)s_scan[w];
  return base + incl - v;
}
__device__ __forceinline__ int block_excl_total(int v, int t, uint32_t* s_scan, int* total) {
  const int incl = wave_incl_scan(v, t);
  __syncthreads();
  if ((t & 63) == 63) s_scan[t >> 6] = (uint32_t)incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < 16; ++w) {
    const int c = (int)s_scan[w];
    if (w < (t >> 6)) base += c;
    tot += c;
  }
  *total = tot;
  return base + incl - v;
}

// a key's bin among 1,024 value-linear bins that descend from `top`
__device__ __forceinline__ int coarse_bin(float v, float top, float scale) {
  return min(1023, max(0, (int)((top - v) * scale)));
}

// The bins' sizes in s_hist (BPT consecutive bins per thread) -> their first positions.  A bin over bin_max
// keys reports its size to *s_big; per_bin(first position, size) sees every bin; returns the position past
// the thread's last bin.
template <int BPT, typename PerBin>
__device__ __forceinline__ int bins_to_positions(uint32_t* s_hist, int t, uint32_t* s_scan, int bin_max,
                                                 int32_t* s_big, PerBin&& per_bin) {
  uint32_t c4[BPT];
  int mine = 0, biggest = 0;
#pragma unroll
  for (int q = 0; q < BPT; ++q) {
    c4[q] = s_hist[t * BPT + q];
    mine += (int)c4[q];
    biggest = max(biggest, (int)c4[q]);
  }
  if (biggest > bin_max) atomicMax(s_big, biggest);
  int at = block_excl(mine, t, s_scan);
#pragma unroll
  for (int q = 0; q < BPT; ++q) {
    s_hist[t * BPT + q] = (uint32_t)at;
    per_bin(at, c4[q]);
    at += (int)c4[q];
  }
  return at;
}

// The binned sorters' two-level histogram of a column — 1,024 value-linear bins over its [min, max] and 1,024
// more over its crowded stretch — and the bin it gives a key.  k_sort_binned and every workgroup of
// k_sort_binned_split build it the same way and must read the same bin off it.
struct BinHistogram {
  uint32_t *coarse, *cum;  // keys per coarse bin of the column, and before it from the top
  uint32_t *fine, *fcum;   // second level: keys per bin of the crowded stretch, and before it inside the stretch
  float cmax, cscale;
  int h_lo, h_hi;  // the crowded stretch: first / last coarse bin over BIN_CROWD keys (h_lo > h_hi: none)
  float ftop, fscale, hull_above;

  // coarse histogram: 1,024 value-linear bins over the column's [min, max] — not mean +- 5 sigma: the columns
  // of a trained table have tails out to 11 sigma, and everything past a clipped range lands in ONE bin
  __device__ __forceinline__ void set_range(float vmin, float vmax) {
    cmax = vmax;
    cscale = vmax > vmin ? 1024.0f / (vmax - vmin) : 0.f;
  }
  __device__ __forceinline__ void count_coarse(float v) { atomicAdd(&coarse[coarse_bin(v, cmax, cscale)], 1u); }
  // Second level.  A fine bin never holds more than the coarse bins it touches, so only CROWDED coarse bins
  // (over BIN_CROWD keys) can overflow one — and they do when the column is a spike plus a few far outliers: the
  // take-off of training, when popular items have grown a hundred times past the untouched rest and mean +- 5
  // sigma puts ten thousand keys into a handful of coarse bins.  The stretch from the first to the last crowded
  // coarse bin gets 1,024 value-linear bins of its own; a key inside it takes its rank from those.
  // (coarse counts complete; s_hull = {1024, -1} before; ends with a barrier)
  __device__ __forceinline__ void find_hull(int t, int32_t* s_hull) {
    const unsigned long long crowded = __ballot(coarse[t] > (uint32_t)BIN_CROWD);
    if ((t & 63) == 0 && crowded != 0ull) {
      atomicMin(&s_hull[0], (t & ~63) + __ffsll(crowded) - 1);
      atomicMax(&s_hull[1], (t & ~63) + 63 - __clzll(crowded));
    }
    __syncthreads();
    h_lo = s_hull[0];
    h_hi = s_hull[1];
    ftop = cmax - (float)h_lo / cscale;  // the stretch's upper edge (any value near it does: membership
    fscale = cscale * (1024.0f / (float)max(h_hi - h_lo + 1, 1));  // is decided by the COARSE bin)
  }
  __device__ __forceinline__ void count_fine(float v, bool on = true) {
    const int cb = coarse_bin(v, cmax, cscale);
    if (on && cb >= h_lo && cb <= h_hi) atomicAdd(&fine[coarse_bin(v, ftop, fscale)], 1u);
  }
  __device__ __forceinline__ void set_hull_above() {  // (cum complete)
    hull_above = h_lo <= h_hi ? (float)cum[h_lo] : 0.f;  // keys above the stretch
  }
  // a key's bin among `bins` equi-depth ones (bscale = bins / n) from its interpolated rank r = (keys above its
  // coarse bin) + (its place inside the bin) x (keys in the bin): monotone in the key, equal keys equal r — bins
  // agree with the order whatever the rounding
  __device__ __forceinline__ int bin_of(float v, int bins, float bscale) const {
    const float x = (cmax - v) * cscale;
    const int cb = min(1023, max(0, (int)x));
    const bool inside = cb >= h_lo && cb <= h_hi;
    const float x2 = (ftop - v) * fscale;
    const int fb = min(1023, max(0, (int)x2));
    const float frac = fminf(fmaxf(inside ? x2 - (float)fb : x - (float)cb, 0.f), 0.999f);
    const float r = inside ? hull_above + ((float)fcum[fb] + frac * (float)fine[fb])
                           : (float)cum[cb] + frac * (float)coarse[cb];
    return min(bins - 1, max(0, (int)(r * bscale)));
  }
};

// A key's place inside its bin, for lane `lane` of the 64-entry window of staged entries at `base`: the first
// position of its bin plus the members that precede it (larger key, or equal key and lower id).  The bin's bounds
// come from the first-of-bin flags of its window (bc), the one before (bp) and the one after (bn) — a bin holds
// <= BIN_MAX = 64 entries; position n_end counts as flagged.  id: the key's own item id, id_at(j): the id staged
// at position j.
template <typename IdAt>
__device__ __forceinline__ int rank_in_window(const uint32_t* s_key, int base, int lane, int n_end,
                                              unsigned long long bp, unsigned long long bc,
                                              unsigned long long bn, int id, IdAt&& id_at) {
  const unsigned long long upto = (2ull << lane) - 1ull;  // bits 0 .. lane
  const int p = base + lane;
  const bool valid = p < n_end;
  const unsigned long long at_or_before = bc & upto, after = bc & ~upto;
  int lo = at_or_before ? base + 63 - __clzll(at_or_before) : base - 1 - __clzll(bp);
  int hi = after ? base + __ffsll(after) - 1 : bn ? base + 63 + __ffsll(bn) : n_end;
  if (!valid) lo = hi = 0;
  const uint32_t u = valid ? s_key[p] : 0u;
  // four members in flight, no bounds tests: an entry past the bin's end belongs to a LATER bin — its key is
  // strictly smaller (equal keys share a bin), so it counts neither as larger nor as equal; the four words
  // past position n_end hold 0, the smallest orderable key
  int rank = 0, equal = 0;
#pragma unroll 1  // (bins hold ~2.5 keys: one or two trips — unrolled further, the remainder tests cost more than the loop)
  for (int j = lo; j < hi; j += 4) {
    const uint32_t o0 = s_key[j], o1 = s_key[j + 1], o2 = s_key[j + 2], o3 = s_key[j + 3];
    rank += (o0 > u ? 1 : 0) + (o1 > u ? 1 : 0) + (o2 > u ? 1 : 0) + (o3 > u ? 1 : 0);
    equal += (o0 == u ? 1 : 0) + (o1 == u ? 1 : 0) + (o2 == u ? 1 : 0) + (o3 == u ? 1 : 0);
  }
  if (equal > 1) {  // equal keys (rare; `equal` counts the key itself once): the lower id goes first
#pragma unroll 1
    for (int j = lo; j < hi; ++j) rank += s_key[j] == u && id_at(j) < id ? 1 : 0;
  }
  return lo + rank;
}

}  // namespace bpr
