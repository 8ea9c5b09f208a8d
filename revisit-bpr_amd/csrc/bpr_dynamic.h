// bpr_dynamic.h — dynamic negative sampling (DNS, Zhang et al., SIGIR 2013): draw M unseen candidates uniformly,
// score them with the model as it is now, train on the highest-scoring one.  ONE device function, sample_dynamic,
// used by k_stream's NEG_DYNAMIC branch (bpr_stream.h) and by the stand-alone kernel (bpr_dynamic.hip); the numpy
// model of it is tests/dynamic_model.py.  DESIGN.md "Dynamic negative sampling" states the draw.
//
//   candidates   sample_uniform's stream: candidate k of triple t is
//                uniform_candidate(draw(seed, t, k >> 2, PURPOSE_UNIFORM, k & 3), I, weights), k < UNIFORM_MAX_CAND
//   accepted     not in seen(u); a_1 .. a_m = the first min(M, accepted) of them in order of k, duplicates kept
//   none         sample_uniform's exact rank pick (the same extra Philox block; item 0 when nothing is unseen)
//   score        <p_u, q_a> (+ bias_a) on the rows the caller's accessor returns
//   pick         best = a_1; a_i replaces it if score(a_i) > score(best), or score(best) is NaN and score(a_i) is not
//
// M = 1 is sample_uniform; so is any M when all scores are equal.
#pragma once
#include "bpr_device.h"

namespace bpr {

// Candidate rows in flight at once: the loads of a chunk of rows are all issued before the first of them is
// reduced.  8 rows at E <= 4 (d <= 256: M = 8 is one round trip, M = 32 four); wider rows keep the chunk at 32
// registers per lane.
template <int E>
constexpr int dynamic_inflight() {
  return E <= 4 ? 8 : (E <= 8 ? 4 : 2);
}

// lane (0..G-1, in its group) of accepted candidate number n (0-based) of a round: the n-th set bit of the group's
// part of the ballot, by halving (5 popcounts).  n past the count: some lane of the group.
__device__ __forceinline__ int nth_set_bit32(uint32_t m, int n) {
  int pos = 0;
#pragma unroll
  for (int w = 16; w >= 1; w >>= 1) {
    const int c = __builtin_popcount((m >> pos) & ((1u << w) - 1u));
    const bool up = n >= c;
    n = up ? n - c : n;
    pos = up ? pos + w : pos;
  }
  return pos;
}
template <int G>
__device__ __forceinline__ int group_count(const Ballot& b, int lane) {
  if constexpr (G == 64) return __builtin_popcount(b.lo) + __builtin_popcount(b.hi);
  else return __builtin_popcount((lane & 32) ? b.hi : b.lo);
}
template <int G>
__device__ __forceinline__ int group_nth_set(const Ballot& b, int n, int lane) {
  if constexpr (G == 64) {
    const int cl = __builtin_popcount(b.lo);
    const bool up = n >= cl;
    return nth_set_bit32(up ? b.hi : b.lo, up ? n - cl : n) + (up ? 32 : 0);
  } else {
    return nth_set_bit32((lane & 32) ? b.hi : b.lo, n);
  }
}

struct DynamicPick {
  int32_t item;
  float score;  // of the pick, as the kernel computed it
  float bias;   // the pick's bias term (0 without a bias)
  int32_t tag;  // what the accessor's load returned for the pick (k_stream: its hot slot, -1 = none)
};

// The first min(M, accepted) accepted candidates of triple t, in order of k: lane s of the group keeps a_{s+1} in
// `mine`; returns how many there are (1 .. M).  None of the 4,096 accepted: sample_uniform's exact pick by rank is a_1.
// Shared with the WARP draw (bpr_warp.h).  All lanes of the wave must call this together (wave-uniform loops).
template <int G, typename Seen>
__device__ __forceinline__ int accepted_candidates(int32_t& mine, const Seen& seen, int64_t n_seen,
                                                   const int32_t* __restrict__ seen_ids, int64_t I, uint64_t seed,
                                                   uint64_t t, int M, int lane, const ItemWeights& iw) {
  static_assert(G >= 32, "lane s of the group keeps accepted candidate s: M <= 32 <= G");
  const int gl = lane & (G - 1);
  mine = 0;
  int cnt = 0;
  constexpr int ROUNDS = UNIFORM_MAX_CAND / G;
  for (int round = 0; round < ROUNDS; ++round) {
    const uint32_t k = (uint32_t)(round * G + gl);
    const uint32_t r = draw(seed, t, k >> 2, PURPOSE_UNIFORM, (int)(k & 3u));
    const int32_t c = uniform_candidate(r, I, iw);
    const Ballot b = wave_ballot(!seen(c));
    const int got = group_count<G>(b, lane);
    const int want = gl - cnt;  // slot gl takes accepted candidate number `want` of this round
    const bool take = gl < M && want >= 0 && want < got;
    const int32_t v = group_bcast<G>(c, group_nth_set<G>(b, take ? want : 0, lane), lane);
    mine = take ? v : mine;
    cnt = min(cnt + got, M);
    if (__all(cnt >= M)) break;
  }
  if (cnt == 0) {  // none of the candidates accepted: sample_uniform's exact pick by rank
    const int64_t n_unseen = (I - 1) - n_seen;
    mine = 0;
    if (n_unseen > 0) {
      const uint32_t r = draw(seed, t, (uint32_t)(UNIFORM_MAX_CAND / 4), PURPOSE_UNIFORM, 0);
      mine = nth_unseen(seen_ids, n_seen, (int64_t)__umulhi(r, (uint32_t)n_unseen));
    }
    cnt = 1;
  }
  return cnt;
}

// The item rows as the caller reads them — Rows has
//   int32_t load(float (&q)[E], float& bias, int32_t item, int gl) const   issues the row's loads, returns a tag
//   void finish(float (&q)[E], int32_t tag, int gl) const                  adds what depends on the tag (hot deltas)
// p[] = the caller's register copy of the user row, q[] receives the chosen row (element layout of bpr_device.h:
// entry e is factor e*G + gl), so the caller does not load q_j again.
// All lanes of the wave must call this together (wave-uniform loops), as sample_uniform.
template <int G, int E, typename Seen, typename Rows>
__device__ __forceinline__ DynamicPick sample_dynamic(float (&q)[E], const float (&p)[E], const Rows& rows,
                                                      const Seen& seen, int64_t n_seen,
                                                      const int32_t* __restrict__ seen_ids, int64_t I, uint64_t seed,
                                                      uint64_t t, int M, int lane, const ItemWeights& iw) {
  const int gl = lane & (G - 1);
  // ---- the first min(M, accepted) accepted candidates, in order of k: lane s of the group keeps a_{s+1}
  int32_t mine;
  const int cnt = accepted_candidates<G>(mine, seen, n_seen, seen_ids, I, seed, t, M, lane, iw);
  // ---- score a_1 .. a_cnt, a chunk of rows in flight at a time, and keep the best
  constexpr int C = dynamic_inflight<E>();
  DynamicPick best = {0, 0.f, 0.f, -1};
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] = 0.f;
  for (int base = 0; base < M; base += C) {
    if (!__any(base < cnt)) break;
    float row[C][E], bias[C];
    int32_t item[C], tag[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      item[c] = group_bcast<G>(mine, (base + c) & (G - 1), lane);
      bias[c] = 0.f;
      tag[c] = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) row[c][e] = 0.f;
      if (base + c < cnt) tag[c] = rows.load(row[c], bias[c], item[c], gl);
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (base + c < cnt) rows.finish(row[c], tag[c], gl);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float s = group_sum<G>(dot<E>(p, row[c]), lane) + bias[c];
      const bool take = base + c < cnt && (base + c == 0 || s > best.score || (best.score != best.score && s == s));
      best.item = take ? item[c] : best.item;
      best.score = take ? s : best.score;
      best.bias = take ? bias[c] : best.bias;
      best.tag = take ? tag[c] : best.tag;
#pragma unroll
      for (int e = 0; e < E; ++e) q[e] = take ? row[c][e] : q[e];
    }
  }
  return best;
}

// the item rows as stored (no hot block: the stand-alone kernels see the table folded)
template <int G, int E>
struct TableRows {
  const float* Q;
  const float* bias;  // the dense item_bias, or NULL
  int d;
  __device__ __forceinline__ int32_t load(float (&q)[E], float& b, int32_t item, int gl) const {
    load_row<G, E>(q, Q + (int64_t)item * d, d, gl);
    if (bias != nullptr) b = bias[item];
    return -1;
  }
  __device__ __forceinline__ void finish(float (&)[E], int32_t, int) const {}
};

}  // namespace bpr
