// bpr_topk.hip — fused scoring + top-K of libbprcore: the k best unseen items of a list of users, with no [n, I]
// score matrix anywhere (bpr_topk_rows / bpr_topk_workspace).
//
// The reference ranks through full logits (example.py:195-230; the preds.jsonl / user-metrics.jsonl savers of
// experiments/options.py:319-351), and revisit_bpr/evaluation.py restates that as P[users] Q^T, a seen scatter and
// torch.topk per block of users: every score goes to HBM and back, and the selection costs three times the GEMM
// (profiles/r06_eval_probe.txt).  Here a workgroup of 256 threads owns 64 users and streams the item table past them
// 128 items x 32 features at a time through LDS into exact f32 MFMA accumulators (v_mfma_f32_32x32x2_f32: items on
// the A side, users on the B side, so a lane's 16 results are 16 items of ONE user).  A score lives in a register
// only long enough to be compared with its row's current k-th best.
//
// Selection.  Every row keeps in LDS a threshold tau = (score, id) — its k-th best at the last compaction — a
// buffer of k + 128 candidates and a count.  After an item tile: (A) every lane counts its scores that beat tau;
// (B) a row whose buffer could overflow is compacted by one wave to its k best, sorted (rank by counting: the
// order "score descending, id ascending" is strict, so ranks are distinct), which tightens tau; (C) scores that
// beat the current tau and are not in the user's sorted seen row (binary search, only for these few) are appended.
// Measured (profiles/recommend_probe.txt): this form LOSES to the composition, 83.5 ms against 63.3 at ML-20M's
// 138,493 users — (C) runs its searches candidate by candidate, each a chain of dependent CSR loads, 32 unrolled
// blocks per lane behind each other.  Next step: test seen membership at compaction, for what was appended since
// the last one, a lane's searches advancing together, so that the tile loop never touches the CSR.
// After the first tiles almost nothing beats tau (~ k ln(I / k) candidates per row over the whole table).  The
// appends race for buffer slots, but what a buffer holds as a SET does not depend on the race, and compaction
// orders it by a strict total order: the output is a pure function of the inputs.
//
// Numerics.  An accumulator is carried through every feature chunk, so s(u, i) is one fmaf chain over the
// features in a fixed order (bpr_topk_shared.h states it, and why it is a contract), the same wherever (u, i) falls
// in a tile, a slice or the user list; features past d are staged as zeros on both sides.  The bias is one fp32 add
// after the chain.
//
// Item slices.  Few users (a serving call, a small evaluation) do not fill the chip: the item tiles are then cut
// into slices, grid = user tiles x slices, each slice writes its sorted top-k to the workspace and k_topk_merge
// merges a row's slices (each entry's rank = its index + binary searches in the other slices).  Layout and sizes:
// bpr_topk_plan.h.  What the other serving kernels use as well — staging, the chain, Cand / better / compact_row —
// is bpr_topk_shared.h; the host prologue the serving entry points share is bpr_serving_host.h, whose
// launch_topk_merge is defined here, beside its kernel.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_item_filter.h"
#include "bpr_serving_host.h"
#include "bpr_topk_plan.h"
#include "bpr_topk_shared.h"

namespace bpr {

struct TopkArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* users;
  int64_t n;
  const int64_t* indptr;
  const int32_t* indices;
  int k, slices;
  int64_t item_tiles;
  float* out_scores;   // [n, slices, k]
  int32_t* out_items;  // [n, slices, k]
};

// VEC: d % 4 == 0 and 16-byte aligned tables (16-byte global loads); else element loads.
// FILT: an item filter (bpr_item_filter.h) lies behind the arguments: an item whose bit is clear is not eligible, and
// the loop walks the slice's non-empty tiles only.  Without it the kernel is what it was before there were filters.
template <bool VEC, bool FILT>
__global__ __launch_bounds__(256) void k_topk(const MaybeFiltered<FILT, TopkArgs> a) {
  constexpr int TU = TOPK_TU, TI = TOPK_TI, LD = TOPK_LD;
  extern __shared__ __align__(16) unsigned char smem[];
  const int cap = a.k + TI;
  float* const sQ = reinterpret_cast<float*>(smem);          // [TI][LD]
  float* const sP = sQ + TI * LD;                            // [TU][LD]
  Cand* const sBuf = reinterpret_cast<Cand*>(sP + TU * LD);  // [TU][cap]
  Cand* const sTau = sBuf + TU * cap;                        // [TU]
  int64_t* const sSeenLo = reinterpret_cast<int64_t*>(sTau + TU);
  int* const sCnt = reinterpret_cast<int*>(sSeenLo + TU);
  int* const sNeed = sCnt + TU;
  int* const sUser = sNeed + TU;
  int* const sSeenLen = sUser + TU;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t u0 = (int64_t)blockIdx.x * TU;
  const int slice = blockIdx.y;
  const int64_t t0 = a.item_tiles * slice / a.slices, t1 = a.item_tiles * (slice + 1) / a.slices;

  if (tid < TU) {
    BPR_STAGE_USER_ROW(u0 + tid, a.n, a.users, a.indptr, a.indices, sUser, sSeenLo, sSeenLen);
    BPR_OPEN_SELECTION_ROW(live, sCnt, sNeed, sTau);
  }
  __syncthreads();

  // the walk (bpr_topk_shared.h).  FILT: the slice's non-empty tiles only.
  auto tile_from = [&](int64_t t) -> int64_t {
    if constexpr (FILT) return filter_next_tile(a.filter, a.I, t, t1);
    else return t;
  };
  const table_tiles items = {a.I};
  BPR_WALK_LANE(a.d, sQ, sP);
  BPR_WALK_TILES_BEGIN(VEC, FILT, tile_from(t0), t1, items, a.Q, a.P, a.d, sUser, sQ, sP, tile_from, walk_nop(),
                       walk_nop())
    // ---- epilogue of the item tile: register q of the lane is item ibase + (q & 3) + 8 (q >> 2) of users r, 32 + r
    const int64_t ibase = t * TI + 32 * w + 4 * h;
    const bool has_bias = a.bias != nullptr;
    float bv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int64_t item = ibase + (q & 3) + 8 * (q >> 2);
      bv[q] = has_bias && item < a.I ? a.bias[item] : 0.f;
    }
    // the wave's word of the filter: bit j is item t * TI + 32 w + j
    uint32_t fw = 0;
    if constexpr (FILT) fw = filter_wave_word(a.filter, a.I, t, __builtin_amdgcn_readfirstlane(w));
    // (A) how many scores beat the row's threshold
    unsigned m0 = 0, m1 = 0;
    {
      const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t item = ibase + (q & 3) + 8 * (q >> 2);
        const bool ok = item > 0 && item < a.I && (!FILT || ((fw >> (4 * h + (q & 3) + 8 * (q >> 2))) & 1u));
        const float s0 = has_bias ? acc0[q] + bv[q] : acc0[q];
        const float s1 = has_bias ? acc1[q] + bv[q] : acc1[q];
        if (ok && better(s0, (int)item, tau0.s, tau0.i)) m0 |= 1u << q;
        if (ok && better(s1, (int)item, tau1.s, tau1.i)) m1 |= 1u << q;
      }
      if (m0) atomicAdd(&sNeed[r], __popc(m0));
      if (m1) atomicAdd(&sNeed[32 + r], __popc(m1));
    }
    __syncthreads();
    // (B) rows whose buffer might not take them all are compacted, which tightens tau
    compact_overflowing_rows(sBuf, sCnt, sNeed, sTau, cap, a.k, w, lane);
    __syncthreads();
    // (C) append what still beats the threshold and the user has not seen
    if (tid < TU) sNeed[tid] = 0;
    if (m0 | m1) {
      const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
      const int32_t* const seen0 = a.indices + sSeenLo[r];
      const int32_t* const seen1 = a.indices + sSeenLo[32 + r];
      const int len0 = sSeenLen[r], len1 = sSeenLen[32 + r];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int item = (int)(ibase + (q & 3) + 8 * (q >> 2));
        if ((m0 >> q) & 1u) {
          const float s0 = has_bias ? acc0[q] + bv[q] : acc0[q];
          if (better(s0, item, tau0.s, tau0.i) && !in_sorted(seen0, len0, item)) {
            const int pos = atomicAdd(&sCnt[r], 1);
            if (pos < cap) sBuf[r * cap + pos] = Cand{s0, item};
          }
        }
        if ((m1 >> q) & 1u) {
          const float s1 = has_bias ? acc1[q] + bv[q] : acc1[q];
          if (better(s1, item, tau1.s, tau1.i) && !in_sorted(seen1, len1, item)) {
            const int pos = atomicAdd(&sCnt[32 + r], 1);
            if (pos < cap) sBuf[(32 + r) * cap + pos] = Cand{s1, item};
          }
        }
      }
    }
  BPR_WALK_TILES_END
  __syncthreads();

  // ---- the slice's result: every row sorted, padded with (-inf, -1)
  for (int row = w; row < TU; row += 4) {
    if (u0 + row >= a.n) break;
    const int c = min(sCnt[row], cap);
    Cand* const buf = sBuf + row * cap;
    if (c > 0) compact_row(buf, c, a.k, lane, &sTau[row], &sCnt[row]);
    const int have = c < a.k ? c : a.k;
    const int64_t out = ((u0 + row) * a.slices + slice) * a.k;
    for (int j = lane; j < a.k; j += 64) {
      const Cand e = j < have ? buf[j] : Cand{-INFINITY, -1};
      a.out_scores[out + j] = e.s;
      a.out_items[out + j] = e.i;
    }
  }
}

// One workgroup per row: S sorted lists of k (padded with id -1 at the end) -> the k best, sorted.
__global__ __launch_bounds__(256) void k_topk_merge(const float* __restrict__ ps, const int32_t* __restrict__ pi, int S,
                                                    int k, float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cand* const sE = reinterpret_cast<Cand*>(smem);  // [S][k]
  int* const sLen = reinterpret_cast<int*>(sE + S * k);
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t base = row * S * k;
  if (tid < S) sLen[tid] = 0;
  __syncthreads();
  for (int e = tid; e < S * k; e += 256) {
    const Cand c = {ps[base + e], pi[base + e]};
    sE[e] = c;
    if (c.i >= 0) atomicAdd(&sLen[e / k], 1);
  }
  __syncthreads();
  int total = 0;
  for (int s = 0; s < S; ++s) total += sLen[s];
  for (int e = tid; e < S * k; e += 256) {
    const int s = e / k, j = e - s * k;
    if (j >= sLen[s]) continue;
    const Cand c = sE[e];
    int rank = j;
    for (int b = 0; b < S && rank < k; ++b) {
      if (b == s) continue;
      const Cand* const L = sE + b * k;
      int lo = 0, hi = sLen[b];  // entries of list b that come before c
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (better(L[mid].s, L[mid].i, c.s, c.i)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      out_s[row * k + rank] = c.s;
      out_i[row * k + rank] = c.i;
    }
  }
  for (int j = (total < k ? total : k) + tid; j < k; j += 256) {
    out_s[row * k + j] = -INFINITY;
    out_i[row * k + j] = -1;
  }
}

int launch_topk_merge(const float* part_s, const int32_t* part_i, int64_t n, int S, int k, size_t merge_lds,
                      float* out_s, int32_t* out_i, hipStream_t stream) {
  if (S <= 1) return BPR_OK;
  return launch_kernel(k_topk_merge, 0, dim3((unsigned)n), dim3(256), merge_lds, stream, part_s, part_i, S, k, out_s,
                       out_i);
}

}  // namespace bpr

extern "C" int bpr_topk_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices,
                                  int64_t* bytes_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_topk_workspace", bytes_host, "bytes_host")) return rc;
  if (int rc = check_topk_shape("bpr_topk_workspace", n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  *bytes_host = topk_workspace_bytes(n, I, k, item_slices);
  return BPR_OK;
}

extern "C" int bpr_topk_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int32_t* slices_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_topk_slices", slices_host, "slices_host")) return rc;
  if (int rc = check_topk_shape("bpr_topk_slices", n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  *slices_host = plan_topk(n, I, k, item_slices).slices;
  return BPR_OK;
}

namespace bpr {
namespace {

// bpr_topk_rows (rows = "_rows", no filter) and bpr_topk_rows_filtered (rows = "_rows_filtered"): one body, the
// messages under the entry point's own name.  The plan does not look at the filter.
int topk_rows(const char* rows, const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
              const int32_t* users, int64_t n, const int64_t* seen_indptr, const int32_t* seen_indices,
              const uint32_t* item_filter, int32_t k, int32_t item_slices, void* workspace, int64_t workspace_bytes,
              int32_t* items_out, float* scores_out, void* hip_stream) {
  const std::string who = std::string("bpr_topk") + rows;
  if (int rc = check_topk_shape(who.c_str(), n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  if (n > 0 && (!P || !Q || !users || !items_out || !scores_out))
    return fail(BPR_ERR_INVALID, who + ": P, Q, users, items_out or scores_out is NULL");
  if (int rc = check_item_filter(who.c_str(), item_filter)) return rc;
  const TopkPlan p = plan_topk(n, I, k, item_slices);
  if (int rc = check_workspace("bpr_topk", workspace, workspace_bytes, p.ws_bytes, nullptr, false, rows)) return rc;
  if (n == 0) return BPR_OK;

  hipStream_t stream = (hipStream_t)hip_stream;
  TopkArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.users = users; a.n = n;
  a.indptr = seen_indptr; a.indices = seen_indices; a.k = k; a.slices = p.slices; a.item_tiles = p.item_tiles;
  slice_outputs(workspace, n, p.slices, k, scores_out, items_out, &a.out_scores, &a.out_items);
  const dim3 grid((unsigned)p.user_tiles, (unsigned)p.slices);
  const bool vec = vec_path(d, P, Q);
  if (item_filter != nullptr) {
    Filtered<TopkArgs> f = {};
    static_cast<TopkArgs&>(f) = a;
    f.filter = item_filter;
    if (int rc = launch_kernel(vec ? k_topk<true, true> : k_topk<false, true>, topk_lds_bytes(TOPK_MAX), grid,
                               dim3(256), p.lds, stream, f))
      return rc;
  } else if (int rc = launch_kernel(vec ? k_topk<true, false> : k_topk<false, false>, topk_lds_bytes(TOPK_MAX), grid,
                                    dim3(256), p.lds, stream, a)) {
    return rc;
  }
  return launch_topk_merge(a.out_scores, a.out_items, n, p.slices, k, p.merge_lds, scores_out, items_out, stream);
}

}  // namespace
}  // namespace bpr

extern "C" int bpr_topk_rows(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                             const int32_t* users, int64_t n, const int64_t* seen_indptr, const int32_t* seen_indices,
                             int32_t k, int32_t item_slices, void* workspace, int64_t workspace_bytes,
                             int32_t* items_out, float* scores_out, void* hip_stream) {
  return bpr::topk_rows("_rows", P, Q, item_bias, I, d, users, n, seen_indptr, seen_indices, nullptr, k, item_slices,
                        workspace, workspace_bytes, items_out, scores_out, hip_stream);
}

extern "C" int bpr_topk_rows_filtered(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                      const int32_t* users, int64_t n, const int64_t* seen_indptr,
                                      const int32_t* seen_indices, const uint32_t* item_filter, int32_t k,
                                      int32_t item_slices, void* workspace, int64_t workspace_bytes,
                                      int32_t* items_out, float* scores_out, void* hip_stream) {
  return bpr::topk_rows("_rows_filtered", P, Q, item_bias, I, d, users, n, seen_indptr, seen_indices, item_filter, k,
                        item_slices, workspace, workspace_bytes, items_out, scores_out, hip_stream);
}

// Test hook, not API (tests/test_item_filter_cpu.py sets its signature): bpr_item_filter.h on host words.  The
// non-empty tiles of each of the `slices` tile ranges [bounds[s], bounds[s + 1]), walked with filter_next_tile:
// counts[s] of them, one slice after the other in tiles[] (room for ceil(I / 128)); empty[t] = filter_tile_empty for
// every tile of the catalogue; and for each of the n_probe ids probe[j]: probe_out[3 j ..] = {word, bit, eligible}.
// Needs no GPU.
extern "C" int bpr_test_filter_tiles(const uint32_t* words, int64_t I, const int64_t* bounds, int32_t slices,
                                     int64_t* tiles, int64_t* counts, uint8_t* empty, const int64_t* probe,
                                     int64_t n_probe, int64_t* probe_out) {
  using namespace bpr;
  if (!words || I < 1 || slices < 0 || reinterpret_cast<uintptr_t>(words) % FILTER_ALIGN != 0)
    return fail(BPR_ERR_INVALID, "bpr_test_filter_tiles: words (16-byte aligned), I >= 1, slices >= 0");
  const int64_t item_tiles = (I + TOPK_TI - 1) / TOPK_TI;
  int64_t at = 0;
  for (int s = 0; s < slices; ++s) {
    if (bounds[s] < 0 || bounds[s] > bounds[s + 1] || bounds[s + 1] > item_tiles)
      return fail(BPR_ERR_INVALID, "bpr_test_filter_tiles: bounds must ascend inside [0, ceil(I / 128)]");
    counts[s] = 0;
    for (int64_t t = filter_next_tile(words, I, bounds[s], bounds[s + 1]); t < bounds[s + 1];
         t = filter_next_tile(words, I, t + 1, bounds[s + 1])) {
      tiles[at++] = t;
      ++counts[s];
    }
  }
  if (empty != nullptr)
    for (int64_t t = 0; t < item_tiles; ++t) empty[t] = filter_tile_empty(words, I, t) ? 1 : 0;
  for (int64_t j = 0; j < n_probe; ++j) {
    probe_out[3 * j] = filter_word_of(probe[j]);
    probe_out[3 * j + 1] = filter_bit_of(probe[j]);
    probe_out[3 * j + 2] = filter_has(words, I, probe[j]) ? 1 : 0;
  }
  return BPR_OK;
}

// Test hook, not API (tests/test_rank_neighbors_filter_cpu.py sets its signature): the `_from` functions of
// bpr_item_filter.h on host words, for a table of N rows and the lower bound `first`.  out_words[wi] =
// filter_word_from for every word; has[i] = filter_has_from for every id 0 .. 32 * words - 1; empty[t] =
// filter_tile_empty_from and next[t] = filter_next_tile_from(t, tiles) for every tile.  Needs no GPU.
extern "C" int bpr_test_filter_words_from(const uint32_t* words, int64_t N, int64_t first, uint32_t* out_words,
                                          uint8_t* has, uint8_t* empty, int64_t* next) {
  using namespace bpr;
  if (!words || N < 1 || first < 0 || reinterpret_cast<uintptr_t>(words) % FILTER_ALIGN != 0)
    return fail(BPR_ERR_INVALID, "bpr_test_filter_words_from: words (16-byte aligned), N >= 1, first >= 0");
  const int64_t nw = filter_words(N), tiles = nw / FILTER_TILE_WORDS;
  for (int64_t wi = 0; wi < nw; ++wi) out_words[wi] = filter_word_from(words, N, wi, first);
  for (int64_t i = 0; i < 32 * nw; ++i) has[i] = filter_has_from(words, N, i, first) ? 1 : 0;
  for (int64_t t = 0; t < tiles; ++t) {
    empty[t] = filter_tile_empty_from(words, N, t, first) ? 1 : 0;
    next[t] = filter_next_tile_from(words, N, t, tiles, first);
  }
  return BPR_OK;
}

// Test hook, not API (tests/test_recommend_cpu.py sets its signature): the plan of a shape.  in = {n, I, d, k,
// item_slices, cus}; out = {slices, user_tiles, item_tiles, tile_users, tile_items, cap, lds, merge_lds, ws_bytes};
// bounds[0 .. slices] = first item of each slice, then I.  Needs no GPU.
extern "C" int bpr_test_topk_plan(const int64_t* in, int64_t* out, int64_t* bounds) {
  using namespace bpr;
  if (int rc = check_topk_shape("bpr_test_topk_plan", in[0], in[1], (int32_t)in[2], (int32_t)in[3], TOPK_MAX,
                                (int32_t)in[4], "I"))
    return rc;
  const TopkPlan p = plan_topk(in[0], in[1], (int)in[3], (int)in[4], in[5] > 0 ? (int)in[5] : TOPK_CUS);
  const int64_t v[] = {p.slices, p.user_tiles, p.item_tiles, TOPK_TU, TOPK_TI, p.cap, (int64_t)p.lds,
                       (int64_t)p.merge_lds, p.ws_bytes};
  memcpy(out, v, sizeof(v));
  slice_bounds(p, topk_slice_tile, TOPK_TI, in[1], bounds);
  return BPR_OK;
}
