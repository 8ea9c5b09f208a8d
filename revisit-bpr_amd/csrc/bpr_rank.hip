// bpr_rank.hip — fused scoring + exact ranking of held-out items (bpr_rank_rows / bpr_rank_workspace): for every
// target of a row, how many eligible items come before it in `recommend`'s order and how many score at least as
// high, with no [n, I] score matrix anywhere.
//
// The reference measures a model through full logits (example.py:195-230; experiments/bpr/exp.py:369-374: every
// metric object argsorts I scores per user; metrics/auc.py:70-130 compares all pairs of a row; metrics/map.py), and
// revisit_bpr/evaluation.py restates that as P[users] Q^T, a seen scatter, torch.topk and bpr_auc_rows over the
// score matrix.  NDCG, Recall, Precision at any cutoff, MAP, MRR and the ROC-AUC are all functions of one quantity:
// the position of each held-out item among the user's unseen items.  Here a workgroup of 256 threads owns 64 rows
// and streams the item table past them with k_topk's tiling (bpr_topk.hip: 128 items x 32 features through LDS,
// v_mfma_f32_32x32x2_f32, a lane holds 16 item scores of one row); a score lives in a register only long enough to
// be placed among its row's few target scores.
//
// Three steps on the caller's stream.
//   1. Target scores (k_rank<.., true>): the concatenated targets of a workgroup's rows are gathered as item tiles
//      and go through the same MFMA routine; of a tile's 128 x 64 results only the (target, owning row) entries are
//      kept.  A target that is not eligible (id outside [1, I), or in the user's seen row) gets score -inf and
//      rank = not_below = -1 here; an eligible one gets its score and 0 / 0.  One launch whatever the slice count,
//      so that every slice sees the same bits.
//   2. Ranking (k_rank<.., false>): every row's live targets (eligible, score not NaN) are sorted in LDS by the
//      result order (rank by counting, as compact_row of bpr_topk_shared.h; duplicates of an id are ordered by their
//      place in the list).  Every streamed eligible score finds by a branch-free binary search the first target it
//      comes before and bumps that bin (runs of one bin are counted privately, as k_auc_rows does); a score equal
//      to that of the targets just in front of its place walks them and bumps their "tied after" counter.  A prefix
//      sum over the bins gives rank, and not_below = rank + tied after.
//   3. With item slices (few rows), grid = row tiles x slices: every slice adds its integer counts to the workspace
//      with vector atomics (integer sums do not depend on the order) and k_rank_finish takes the prefix sums.
//
// Seen exclusion never searches the CSR per candidate (the loss recorded in bpr_topk.hip's header).  Four threads
// share a row's sorted seen list, entries e = sub (mod 4) each; a thread keeps its next entry in a register, found
// by one binary search at the slice's first tile, and per item tile sets the bits of the entries that fall into the
// tile in a 128-bit mask per row in LDS.  CSR traffic: one read of each row's seen list per slice.
//
// Numerics: k_topk's — the same staging and the same chain (bpr_topk_shared.h), one accumulator carried through
// every feature chunk, zeros past d, the bias one fp32 add afterwards — so a score's bits are k_topk's for the same
// pair, wherever the pair falls.
//
// Not measured against the composition until tools/rank_probe.py has run on the chip (profiles/rank_probe.txt).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <atomic>
#include <string>

#include "bpr_item_filter.h"
#include "bpr_rank_plan.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {

static_assert(RANK_KC == TOPK_KC && RANK_LD == TOPK_LD, "k_rank stages k_topk's chunks (bpr_topk_shared.h)");
static_assert(RANK_TI == TOPK_TI, "an item tile of k_rank is a tile of the item filter (bpr_item_filter.h)");

struct RankArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* users;
  int64_t n;
  const int64_t* tptr;     // [n + 1]
  const int32_t* titems;
  const int64_t* indptr;   // seen CSR or NULL
  const int32_t* indices;
  int slices;
  int64_t item_tiles;
  int32_t* rank;
  int32_t* not_below;
  float* score;
  int32_t* ws;  // slices > 1: [3][n][RANK_TMAX]
};

__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ v, int len, int64_t x) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave: the T <= RANK_TMAX targets of a row -> its live ones sorted into L, their places in the list into perm,
// the row's counters zeroed, *cnt = how many are live.  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ void sort_row(const RankArgs& a, int64_t tlo, int T, int lane, Cand* L, uint16_t* perm,
                                         int* ht, int* cnt) {
  Cand* const tmp = reinterpret_cast<Cand*>(ht);  // (staged through the counters' LDS: 2 T <= RANK_HT ints)
  Cand e[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int p = lane + 64 * q;
    e[q] = Cand{0.f, -1};
    if (p < T) {
      const float s = a.score[tlo + p];
      const bool live = a.rank[tlo + p] == 0 && s == s;
      e[q] = Cand{s, live ? a.titems[tlo + p] : -1};
      tmp[p] = e[q];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int pos[2] = {0, 0};
  for (int j = 0; j < T; ++j) {
    const Cand o = tmp[j];
    if (o.i < 0) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      pos[q] += (better(o.s, o.i, e[q].s, e[q].i) || (o.s == e[q].s && o.i == e[q].i && j < lane + 64 * q)) ? 1 : 0;
  }
  const int live = __popcll(__ballot(e[0].i >= 0)) + __popcll(__ballot(e[1].i >= 0));
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (e[q].i >= 0) {
      L[pos[q]] = e[q];
      perm[pos[q]] = (uint16_t)(lane + 64 * q);
    }
  }
  for (int x = lane; x < RANK_HT; x += 64) ht[x] = 0;
  if (lane == 0) *cnt = live;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// VEC: d % 4 == 0 and 16-byte aligned tables (16-byte global loads); else element loads.
// PRE: the target-score pass (step 1 of the header); else the ranking pass (step 2).
// FILT: an item filter (bpr_item_filter.h) lies behind the arguments: an item whose bit is clear is not eligible.  The
// target pass tests the target's own bit; the ranking pass joins the tile's four words with the seen mask and walks
// the slice's non-empty tiles only.  Without it the kernel is what it was before there were filters.
template <bool VEC, bool PRE, bool FILT>
__global__ __launch_bounds__(256) void k_rank(const MaybeFiltered<FILT, RankArgs> a) {
  constexpr bool SKIP = FILT && !PRE;  // the walk leaves out the empty tiles
  constexpr int TR = RANK_TR, TI = RANK_TI, KC = RANK_KC, LD = RANK_LD, TM = RANK_TMAX, HT = RANK_HT;
  extern __shared__ __align__(16) unsigned char smem[];
  float* const sQ = reinterpret_cast<float*>(smem);  // [TI][LD]
  float* const sP = sQ + TI * LD;                    // [TR][LD]
  int64_t* const sSeenLo = reinterpret_cast<int64_t*>(sP + TR * LD);  // [TR]
  int64_t* const sTgtLo = sSeenLo + TR;              // [TR + 1] (+ one pad: the largest live count)
  int* const sMaxT = reinterpret_cast<int*>(sTgtLo + TR + 1);
  int* const sUser = reinterpret_cast<int*>(sTgtLo + TR + 2);
  int* const sSeenLen = sUser + TR;
  int* const sT = sSeenLen + TR;
  int* const sOwner = sT + TR;                                   // PRE: [TI]
  uint32_t* const sMask = reinterpret_cast<uint32_t*>(sT + TR);  // ranking: [TR][4], bit set = seen
  Cand* const sL = reinterpret_cast<Cand*>(sMask + TR * 4);    // [TR][TM]
  int* const sHT = reinterpret_cast<int*>(sL + TR * TM);         // [TR][HT]
  uint16_t* const sPerm = reinterpret_cast<uint16_t*>(sHT + TR * HT);  // [TR][TM]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * TR;
  const int slice = blockIdx.y;

  if (tid < TR) {
    const int64_t row = r0 + tid;
    const bool live = row < a.n;
    const int u = live ? a.users[row] : -1;
    int64_t lo = 0;
    int len = 0;
    if (live && a.indptr != nullptr && a.indices != nullptr) {
      lo = a.indptr[u];
      len = (int)(a.indptr[u + 1] - lo);
    }
    const int64_t tlo = a.tptr[live ? row : a.n];
    sUser[tid] = u;
    sSeenLo[tid] = lo;
    sSeenLen[tid] = len;
    sTgtLo[tid] = tlo;
    const int64_t cnt = live ? a.tptr[row + 1] - tlo : 0;
    sT[tid] = cnt < 0 ? 0 : cnt > TM ? TM : (int)cnt;
    if (tid == 0) {
      sTgtLo[TR] = a.tptr[r0 + TR < a.n ? r0 + TR : a.n];
      *sMaxT = 0;
    }
  }
  __syncthreads();

  // item tiles this workgroup walks: PRE, the targets of its rows in tiles of TI; else its slice of the table
  const int64_t g0 = sTgtLo[0], g1 = sTgtLo[TR];
  int64_t t0, t1;
  if (PRE) {
    t0 = 0;
    t1 = (g1 - g0 + TI - 1) / TI;
  } else {
    t0 = a.item_tiles * slice / a.slices;
    t1 = a.item_tiles * (slice + 1) / a.slices;
  }
  // the item staged as row `row` of tile t (-1: zeros)
  auto item_of = [&](int64_t t, int row) -> int64_t {
    if (PRE) {
      const int64_t p = g0 + t * TI + row;
      if (p >= g1) return -1;
      const int id = a.titems[p];
      return id >= 1 && id < a.I ? id : -1;
    }
    const int64_t item = t * TI + row;
    return item < a.I ? item : -1;
  };

  int top = 0;  // ranking: the first step of the binary search (largest power of two <= the longest list)
  const int32_t* seen = nullptr;  // ranking: this thread's quarter of row tid >> 2's seen list
  int se = 0, slen = 0, snext = INT_MAX;
  // The walk: the contract is the head of bpr_topk_shared.h; the loop is this kernel's own copy of BPR_WALK_TILES_BEGIN
  // (why: there).  SKIP: the slice's non-empty tiles only.
  auto tile_from = [&](int64_t t) -> int64_t {
    if constexpr (SKIP) return filter_next_tile(a.filter, a.I, t, t1);
    else return t;
  };
  int64_t tn = 0;
  auto next = [&](int64_t t) -> int64_t { return SKIP ? tn : t + 1; };
  int64_t first = t0;
  if (!PRE) {
    for (int row = w; row < TR; row += 4) {
      sort_row(a, sTgtLo[row], sT[row], lane, sL + row * TM, sPerm + row * TM, sHT + row * HT, &sT[row]);
      if (lane == 0) atomicMax(sMaxT, sT[row]);
    }
    __syncthreads();
    const int maxT = *sMaxT;
    if (maxT == 0) t1 = t0;  // no live target in these rows: nothing to count
    top = 1;
    while (top <= maxT) top <<= 1;
    top >>= 1;
    first = tile_from(t0);  // (after t1 is final)
    const int row = tid >> 2;
    slen = sSeenLen[row];
    if (slen > 0 && first < t1) {
      seen = a.indices + sSeenLo[row];
      se = lower_bound_i32(seen, slen, first * TI) + (tid & 3);
      snext = se < slen ? seen[se] : INT_MAX;
    }
  }

  // the next chunk travels global -> registers while the current one is multiplied, then registers -> LDS
  float4 qreg[4], preg[2];
  auto fetch = [&](int64_t t, int c) {
    const int kc = c * KC;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int f = tid + 256 * m, row = f >> 3, kk = kc + 4 * (f & 7);
      const int64_t item = item_of(t, row);
      qreg[m] = item >= 0 ? load4<VEC>(a.Q + item * a.d, kk, a.d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int f = tid + 256 * m, row = f >> 3, kk = kc + 4 * (f & 7);
      const int u = sUser[row];
      preg[m] = u >= 0 ? load4<VEC>(a.P + (int64_t)u * a.d, kk, a.d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
    BPR_STASH_CHUNK(sQ, qreg, 4, tid, 256);
    BPR_STASH_CHUNK(sP, preg, 2, tid, 256);
  };

  const int nch = (a.d + KC - 1) / KC;
  const float* const qa = sQ + (32 * w + r) * LD + 4 * h;
  const float* const pb0 = sP + r * LD + 4 * h;
  const float* const pb1 = sP + (32 + r) * LD + 4 * h;
  const bool has_bias = a.bias != nullptr;
  if (first < t1) fetch(first, 0);
  for (int64_t t = first; t < t1; t = next(t)) {
    if constexpr (SKIP) tn = tile_from(t + 1);
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
    for (int c = 0; c < nch; ++c) {
      __syncthreads();
      stash();
      if (c == 0) {  // (the epilogue of the tile before has passed the barrier above)
        if (PRE) {
          if (tid < TI) {  // the row that owns target g0 + t TI + tid: tgt_lo[row] <= p < tgt_lo[row + 1]
            const int64_t p = g0 + t * TI + tid;
            int lo = 0, hi = TR;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (sTgtLo[mid + 1] <= p) lo = mid + 1; else hi = mid;
            }
            sOwner[tid] = p < g1 && lo < TR ? lo : -1;
          }
        } else {
          sMask[tid] = 0u;
        }
      }
      __syncthreads();
      if (!PRE && c == 0) {  // the seen entries of this thread's quarter that fall into the tile
        const int64_t hi = (t + 1) * TI;
        if constexpr (SKIP) {
          // A run of skipped tiles may lie behind: the cursor goes to the first entry of ITS residue class (mod 4)
          // that is at or past this tile, by one search, not entry by entry.  Every thread keeps its class, so the
          // four still cover every entry once (tests/test_rank_neighbors_filter_cpu.py models the rule).
          if (snext < t * TI) {
            const int at = lower_bound_i32(seen, slen, t * TI);  // > se: seen[se] is below the tile
            se += (at - se + 3) & ~3;
            snext = se < slen ? seen[se] : INT_MAX;
          }
        }
        while (snext < hi) {
          const int li = snext - (int)(t * TI);  // (negative only for a row that is not sorted: passed over)
          if (li >= 0) atomicOr(&sMask[(tid >> 2) * 4 + (li >> 5)], 1u << (li & 31));
          se += 4;
          snext = se < slen ? seen[se] : INT_MAX;
        }
      }
      if (c + 1 < nch) fetch(t, c + 1);
      else if (next(t) < t1) fetch(next(t), 0);
      mfma_chunk2(qa, pb0, pb1, acc0, acc1);
    }
    __syncthreads();  // the tile's owners / seen masks are complete

    // ---- epilogue of the tile: register q of the lane is staged row lbase + (q & 3) + 8 (q >> 2), rows r, 32 + r
    const int lbase = 32 * w + 4 * h;
    if (PRE) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int li = lbase + (q & 3) + 8 * (q >> 2);
        const int own = sOwner[li];
        if (own < 0 || (own & 31) != r) continue;
        const int64_t p = g0 + t * TI + li;
        const int id = a.titems[p];
        const bool valid = id >= 1 && id < a.I;
        float s = own == r ? acc0[q] : acc1[q];
        if (has_bias && valid) s = s + a.bias[id];
        bool ok = valid;
        if (ok && sSeenLen[own] > 0) {
          const int32_t* const v = a.indices + sSeenLo[own];
          const int at = lower_bound_i32(v, sSeenLen[own], id);
          ok = !(at < sSeenLen[own] && v[at] == id);
        }
        if constexpr (FILT) ok = ok && ((filter_word(a.filter, a.I, filter_word_of(id)) >> filter_bit_of(id)) & 1u);
        a.score[p] = ok ? s : -INFINITY;
        a.rank[p] = ok ? 0 : -1;
        a.not_below[p] = ok ? 0 : -1;
      }
    } else {
      const int64_t ibase = t * TI + lbase;
      uint32_t seen0 = sMask[r * 4 + w], seen1 = sMask[(32 + r) * 4 + w];
      if constexpr (FILT) {  // eligible = not seen AND the wave's word of the filter (wave-uniform: a scalar load)
        const uint32_t fw = filter_wave_word(a.filter, a.I, t, __builtin_amdgcn_readfirstlane(w));
        seen0 |= ~fw;
        seen1 |= ~fw;
      }
      const int T0 = sT[r], T1 = sT[32 + r];
      const Cand* const L0 = sL + r * TM;
      const Cand* const L1 = sL + (32 + r) * TM;
      float s0[16], s1[16];
      int p0[16], p1[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t item = ibase + (q & 3) + 8 * (q >> 2);
        const float bv = has_bias && item < a.I ? a.bias[item] : 0.f;
        s0[q] = has_bias ? acc0[q] + bv : acc0[q];
        s1[q] = has_bias ? acc1[q] + bv : acc1[q];
        p0[q] = p1[q] = 0;
      }
      // place = how many targets of the row the item does NOT come before (they are the first ones of the list)
      for (int step = top; step > 0; step >>= 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int item = (int)(ibase + (q & 3) + 8 * (q >> 2));
          const int c0 = p0[q] + step, c1 = p1[q] + step;
          if (c0 <= T0) {
            const Cand e = L0[c0 - 1];
            if (!better(s0[q], item, e.s, e.i)) p0[q] = c0;
          }
          if (c1 <= T1) {
            const Cand e = L1[c1 - 1];
            if (!better(s1[q], item, e.s, e.i)) p1[q] = c1;
          }
        }
      }
      int* const ht0 = sHT + r * HT;
      int* const ht1 = sHT + (32 + r) * HT;
      int rb0 = -1, rc0 = 0, rb1 = -1, rc1 = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int bit = 4 * h + (q & 3) + 8 * (q >> 2);
        const int64_t item64 = ibase + (q & 3) + 8 * (q >> 2);
        const int item = (int)item64;
        const bool inside = item64 > 0 && item64 < a.I;
        if (inside && T0 > 0 && !((seen0 >> bit) & 1u)) {
          const int at = p0[q];
          if (at < T0) {
            if (at == rb0) {
              ++rc0;
            } else {
              if (rc0) atomicAdd(&ht0[rb0], rc0);
              rb0 = at;
              rc0 = 1;
            }
          }
          for (int x = at - 1; x >= 0 && L0[x].s == s0[q]; --x)
            if (L0[x].i != item) atomicAdd(&ht0[TM + 2 + x], 1);
        }
        if (inside && T1 > 0 && !((seen1 >> bit) & 1u)) {
          const int at = p1[q];
          if (at < T1) {
            if (at == rb1) {
              ++rc1;
            } else {
              if (rc1) atomicAdd(&ht1[rb1], rc1);
              rb1 = at;
              rc1 = 1;
            }
          }
          for (int x = at - 1; x >= 0 && L1[x].s == s1[q]; --x)
            if (L1[x].i != item) atomicAdd(&ht1[TM + 2 + x], 1);
        }
      }
      if (rc0) atomicAdd(&ht0[rb0], rc0);
      if (rc1) atomicAdd(&ht1[rb1], rc1);
    }
  }
  if (PRE) return;
  __syncthreads();

  // ---- the slice's counts: one slice writes the result, several add to the workspace
  for (int row = w; row < TR; row += 4) {
    if (r0 + row >= a.n) break;
    const int T = sT[row];
    const int* const ht = sHT + row * HT;
    const uint16_t* const perm = sPerm + row * TM;
    const int64_t tlo = sTgtLo[row];
    for (int x = lane; x < T; x += 64) {
      if (a.slices == 1) {
        int before = 0;
        for (int b = 0; b <= x; ++b) before += ht[b];
        a.rank[tlo + perm[x]] = before;
        a.not_below[tlo + perm[x]] = before + ht[TM + 2 + x];
      } else {
        const int64_t at = (r0 + row) * TM + x;
        if (ht[x]) atomicAdd(&a.ws[at], ht[x]);
        if (ht[TM + 2 + x]) atomicAdd(&a.ws[a.n * TM + at], ht[TM + 2 + x]);
        if (slice == 0) a.ws[2 * a.n * TM + at] = perm[x];
      }
    }
  }
}

// Several slices: entry x of row `row` (place -1: the row has fewer live targets) -> rank = bins 0 .. x summed.
__global__ __launch_bounds__(256) void k_rank_finish(const int32_t* __restrict__ ws, int64_t n,
                                                     const int64_t* __restrict__ tptr, int32_t* __restrict__ rank,
                                                     int32_t* __restrict__ not_below) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n * RANK_TMAX) return;
  const int place = ws[2 * n * RANK_TMAX + at];
  if (place < 0) return;
  const int64_t row = at / RANK_TMAX;
  int before = 0;
  for (int64_t b = row * RANK_TMAX; b <= at; ++b) before += ws[b];
  rank[tptr[row] + place] = before;
  not_below[tptr[row] + place] = before + ws[n * RANK_TMAX + at];
}

// out[0] = the longest row of tgt_indptr, out[1] = 1 if a row has a negative length
__global__ __launch_bounds__(256) void k_rank_check(const int64_t* __restrict__ tptr, int64_t n, int32_t* out) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int64_t len = tptr[row + 1] - tptr[row];
  if (len < 0) atomicMax(out + 1, 1);
  else atomicMax(out, len > INT_MAX ? INT_MAX : (int32_t)len);
}

// the check's two words: a ring of slots, so that calls on different streams do not share one
constexpr int RANK_CHECK_SLOTS = 64;
__device__ int32_t g_rank_check[RANK_CHECK_SLOTS * 2];
static std::atomic<unsigned> g_rank_check_next{0};

static int check_shape(const char* who, int64_t n, int64_t I, int32_t d, int32_t item_slices) {
  if (int rc = check_table_shape(who, n, I, d, "I")) return rc;
  if (int rc = check_item_slices(who, item_slices, RANK_MAX_SLICES)) return rc;
  if (n > 0x7FFFFFFF / RANK_TMAX)  // (the finish kernel's grid: n * RANK_TMAX / 256 workgroups)
    return fail(BPR_ERR_INVALID, std::string(who) + ": n must be below 2^31 / " + std::to_string(RANK_TMAX));
  return BPR_OK;
}

// item_filter NULL: the instantiation without a filter, with the arguments as they were
template <bool PRE>
static int launch_rank(const RankArgs& a, const uint32_t* item_filter, dim3 grid, size_t lds, bool vec,
                       hipStream_t stream) {
  if (item_filter != nullptr) {
    Filtered<RankArgs> f = {};
    static_cast<RankArgs&>(f) = a;
    f.filter = item_filter;
    return launch_kernel(vec ? k_rank<true, PRE, true> : k_rank<false, PRE, true>, rank_lds_bytes(), grid, dim3(256),
                         lds, stream, f);
  }
  return launch_kernel(vec ? k_rank<true, PRE, false> : k_rank<false, PRE, false>, rank_lds_bytes(), grid, dim3(256),
                       lds, stream, a);
}

}  // namespace bpr

extern "C" int bpr_rank_workspace(int64_t n, int64_t I, int32_t d, int32_t item_slices, int64_t* bytes_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_rank_workspace", bytes_host, "bytes_host")) return rc;
  if (int rc = check_shape("bpr_rank_workspace", n, I, d, item_slices)) return rc;
  *bytes_host = rank_workspace_bytes(n, I, item_slices);
  return BPR_OK;
}

extern "C" int bpr_rank_slices(int64_t n, int64_t I, int32_t d, int32_t item_slices, int32_t* slices_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_rank_slices", slices_host, "slices_host")) return rc;
  if (int rc = check_shape("bpr_rank_slices", n, I, d, item_slices)) return rc;
  *slices_host = plan_rank(n, I, item_slices).slices;
  return BPR_OK;
}

namespace bpr {
namespace {

// bpr_rank_rows (rows = "_rows", no filter) and bpr_rank_rows_filtered (rows = "_rows_filtered"): one body, the
// messages under the entry point's own name.  The plan does not look at the filter.
int rank_rows(const char* rows, const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
              const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
              const int64_t* seen_indptr, const int32_t* seen_indices, const uint32_t* item_filter,
              int32_t item_slices, void* workspace, int64_t workspace_bytes, int32_t* rank_out, int32_t* not_below_out,
              float* score_out, void* hip_stream) {
  const std::string who = std::string("bpr_rank") + rows;
  if (int rc = check_shape(who.c_str(), n, I, d, item_slices)) return rc;
  if (n > 0 && (!P || !Q || !users || !tgt_indptr))
    return fail(BPR_ERR_INVALID, who + ": P, Q, users or tgt_indptr is NULL");
  if (int rc = check_item_filter(who.c_str(), item_filter)) return rc;
  const RankPlan p = plan_rank(n, I, item_slices);
  if (int rc = check_workspace("bpr_rank", workspace, workspace_bytes, p.ws_bytes, nullptr, false, rows)) return rc;
  if (n == 0) return BPR_OK;

  hipStream_t stream = (hipStream_t)hip_stream;
  // the one host read: the two ends of tgt_indptr and the longest row (a row past RANK_TMAX is refused, not run)
  int32_t* check = nullptr;
  BPR_HIP_CHECK(hipGetSymbolAddress(reinterpret_cast<void**>(&check), HIP_SYMBOL(g_rank_check)));
  check += 2 * (g_rank_check_next.fetch_add(1) % RANK_CHECK_SLOTS);
  BPR_HIP_CHECK(hipMemsetAsync(check, 0, 2 * sizeof(int32_t), stream));
  hipLaunchKernelGGL(k_rank_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tgt_indptr, n, check);
  BPR_HIP_CHECK(hipGetLastError());
  int64_t ends[2] = {0, 0};
  int32_t lens[2] = {0, 0};
  BPR_HIP_CHECK(hipMemcpyAsync(&ends[0], tgt_indptr, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  BPR_HIP_CHECK(hipMemcpyAsync(&ends[1], tgt_indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  BPR_HIP_CHECK(hipMemcpyAsync(lens, check, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  BPR_HIP_CHECK(hipStreamSynchronize(stream));
  if (ends[0] < 0 || ends[1] < ends[0] || lens[1] != 0)
    return fail(BPR_ERR_INVALID, who + ": tgt_indptr does not ascend");
  if (lens[0] > RANK_TMAX)
    return fail(BPR_ERR_INVALID, who + ": a row holds " + std::to_string(lens[0]) + " targets, at most " +
                                     std::to_string(RANK_TMAX) + " (RANK_TMAX) fit: split the row");
  if (ends[1] == ends[0]) return BPR_OK;
  if (!tgt_items || !rank_out || !not_below_out || !score_out)
    return fail(BPR_ERR_INVALID, who + ": tgt_items, rank_out, not_below_out or score_out is NULL");

  RankArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.users = users; a.n = n; a.tptr = tgt_indptr;
  a.titems = tgt_items; a.indptr = seen_indptr; a.indices = seen_indices; a.slices = p.slices;
  a.item_tiles = p.item_tiles; a.rank = rank_out; a.not_below = not_below_out; a.score = score_out;
  a.ws = reinterpret_cast<int32_t*>(workspace);
  const bool vec = vec_path(d, P, Q);
  if (int rc = launch_rank<true>(a, item_filter, dim3((unsigned)p.row_tiles), p.pre_lds, vec, stream)) return rc;
  if (p.slices > 1) {  // bins and tied after: 0; place in the list: -1
    const size_t third = (size_t)n * RANK_TMAX * sizeof(int32_t);
    BPR_HIP_CHECK(hipMemsetAsync(a.ws, 0, 2 * third, stream));
    BPR_HIP_CHECK(hipMemsetAsync(a.ws + 2 * n * RANK_TMAX, 0xFF, third, stream));
  }
  if (int rc = launch_rank<false>(a, item_filter, dim3((unsigned)p.row_tiles, (unsigned)p.slices), p.lds, vec, stream)) return rc;
  if (p.slices > 1) {
    hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)((n * RANK_TMAX + 255) / 256)), dim3(256), 0, stream, a.ws, n,
                       tgt_indptr, rank_out, not_below_out);
    BPR_HIP_CHECK(hipGetLastError());
  }
  return BPR_OK;
}

}  // namespace
}  // namespace bpr

extern "C" int bpr_rank_rows(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                             const int32_t* users, int64_t n, const int64_t* tgt_indptr, const int32_t* tgt_items,
                             const int64_t* seen_indptr, const int32_t* seen_indices, int32_t item_slices,
                             void* workspace, int64_t workspace_bytes, int32_t* rank_out, int32_t* not_below_out,
                             float* score_out, void* hip_stream) {
  return bpr::rank_rows("_rows", P, Q, item_bias, I, d, users, n, tgt_indptr, tgt_items, seen_indptr, seen_indices,
                        nullptr, item_slices, workspace, workspace_bytes, rank_out, not_below_out, score_out,
                        hip_stream);
}

extern "C" int bpr_rank_rows_filtered(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                      const int32_t* users, int64_t n, const int64_t* tgt_indptr,
                                      const int32_t* tgt_items, const int64_t* seen_indptr,
                                      const int32_t* seen_indices, const uint32_t* item_filter, int32_t item_slices,
                                      void* workspace, int64_t workspace_bytes, int32_t* rank_out,
                                      int32_t* not_below_out, float* score_out, void* hip_stream) {
  return bpr::rank_rows("_rows_filtered", P, Q, item_bias, I, d, users, n, tgt_indptr, tgt_items, seen_indptr,
                        seen_indices, item_filter, item_slices, workspace, workspace_bytes, rank_out, not_below_out,
                        score_out, hip_stream);
}

// Test hook, not API (tests/test_rank_cpu.py sets its signature): the plan of a shape.  in = {n, I, d, item_slices,
// cus}; out = {slices, row_tiles, item_tiles, tile_rows, tile_items, tmax, lds, pre_lds, ws_bytes};
// bounds[0 .. slices] = first item of each slice, then I.  Needs no GPU.
extern "C" int bpr_test_rank_plan(const int64_t* in, int64_t* out, int64_t* bounds) {
  using namespace bpr;
  if (int rc = check_shape("bpr_test_rank_plan", in[0], in[1], (int32_t)in[2], (int32_t)in[3])) return rc;
  const RankPlan p = plan_rank(in[0], in[1], (int)in[3], in[4] > 0 ? (int)in[4] : RANK_CUS);
  const int64_t v[] = {p.slices, p.row_tiles, p.item_tiles, RANK_TR, RANK_TI, RANK_TMAX, (int64_t)p.lds,
                       (int64_t)p.pre_lds, p.ws_bytes};
  memcpy(out, v, sizeof(v));
  slice_bounds(p, rank_slice_tile, RANK_TI, in[1], bounds);
  return BPR_OK;
}
