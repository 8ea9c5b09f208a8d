// bpr_scored.h — the two samplers that score unseen candidates with the model as it is now.  ONE device function,
// sample_scored<G, E, KIND>, used by k_stream's scored branch (bpr_stream.h) and by the stand-alone kernel
// k_sample_scored (bpr_dynamic.hip); the numpy models of it are tests/dynamic_model.py and tests/warp_model.py.
//
// Both kinds
//   candidates   sample_uniform's stream: candidate k of triple t is
//                uniform_candidate(draw(seed, t, k >> 2, PURPOSE_UNIFORM, k & 3), I, weights), k < UNIFORM_MAX_CAND
//   accepted     not in seen(u); a_1 .. a_m = the first min(K, accepted) of them in order of k, duplicates kept
//   none         sample_uniform's exact rank pick (the same extra Philox block; item 0 when nothing is unseen)
//   score        <p_u, q_a> (+ bias_a) on the rows the caller's accessor returns
//
// NEG_DYNAMIC — dynamic negative sampling (DNS, Zhang et al., SIGIR 2013): train on the highest-scoring of K = M
// candidates.  DESIGN.md §4.16 states the draw.
//   pick         best = a_1; a_i replaces it if score(a_i) > score(best), or score(best) is NaN and score(a_i) is not
// M = 1 is sample_uniform; so is any M when all scores are equal.
//
// NEG_WARP — the WARP objective (Weston, Bengio, Usunier: "WSABIE", IJCAI 2011; LightFM's default loss): try up to
// K = N candidates until one violates the margin, estimate the positive's rank from how many draws that took, weight
// the step by log(rank), skip the triple when nothing violates.  DESIGN.md §4.17 states the draw.
//   scores       x_i = <p_u, q_i> (+ b_i), x_k = <p_u, q_{a_k}> (+ b_{a_k})
//   violator     the smallest k with x_k > x_i - margin (a NaN on either side compares false); tries = k
//   none         the triple is SKIPPED: item -1, tries 0
//   weight       L = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - |seen(u)|
// N = 1 on a user whose every unseen item violates is sample_uniform.
#pragma once
#include "bpr_device.h"
#include "bpr_scored_plan.h"

namespace bpr {

static_assert(NEG_DYNAMIC == BPR_NEG_DYNAMIC && NEG_WARP == BPR_NEG_WARP,
              "the kernels' template argument is the ABI's sampler kind");

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

// The first min(K, accepted) accepted candidates of triple t, in order of k: lane s of the group keeps a_{s+1} in
// `mine`; returns how many there are (1 .. K).  None of the 4,096 accepted: sample_uniform's exact pick by rank is a_1.
// All lanes of the wave must call this together (wave-uniform loops).
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

struct ScoredPick {
  int32_t item;   // the pick; NEG_WARP: the violator, -1 = the triple is skipped
  int32_t tries;  // NEG_WARP: k of the violator, 0 = skipped
  float x_pos;    // NEG_WARP: x_i as the kernel computed it
  float x_neg;    // the pick's score as the kernel computed it (NEG_WARP: 0 when skipped)
  float bias_pos, bias_neg;  // NEG_WARP: the positive's bias term; the pick's (0 without a bias)
  int32_t tag;    // what the accessor's load returned for the pick (k_stream: its hot slot, -1 = none)
  float weight;   // NEG_WARP: L (0 when skipped)
};

__device__ __forceinline__ float warp_weight(int64_t n_unseen, int tries) {
  const int64_t r = n_unseen / (int64_t)tries;
  return logf((float)(r > 1 ? r : 1));
}

// The item rows as the caller reads them — Rows has
//   int32_t load(float (&q)[E], float& bias, int32_t item, int gl) const   issues the row's loads, returns a tag
//   void finish(float (&q)[E], int32_t tag, int gl) const                  adds what depends on the tag (hot deltas)
// p[] = the caller's register copy of the user row, q[] receives the chosen row (element layout of bpr_device.h:
// entry e is factor e*G + gl), so the caller does not load q_j again.  NEG_WARP: qi[] receives the row of the
// positive `pos` (finish() applied), so the caller loads neither again; NEG_DYNAMIC leaves qi, pos and margin alone.
// The rows are loaded a chunk of dynamic_inflight_rows(E) at a time, all of a chunk's loads issued before the first
// reduction — NEG_WARP: q_i's with the first chunk, x_i has to be known before the first comparison, and no chunk
// past the one with the violator is loaded.
// All lanes of the wave must call this together (wave-uniform loops), as sample_uniform: the groups of a wave walk
// their chunks in lockstep until each has run out of candidates (NEG_WARP: or has its violator).
template <int G, int E, int KIND, typename Seen, typename Rows>
__device__ __forceinline__ ScoredPick sample_scored(float (&qi)[E], float (&q)[E], const float (&p)[E],
                                                    const Rows& rows, int32_t pos, const Seen& seen, int64_t n_seen,
                                                    const int32_t* __restrict__ seen_ids, int64_t I, uint64_t seed,
                                                    uint64_t t, int K, float margin, int lane,
                                                    const ItemWeights& iw) {
  static_assert(KIND == NEG_DYNAMIC || KIND == NEG_WARP, "a scored kind");
  constexpr bool WARP = KIND == NEG_WARP;
  const int gl = lane & (G - 1);
  // ---- the first min(K, accepted) accepted candidates, in order of k: lane s of the group keeps a_{s+1}
  int32_t mine;
  const int cnt = accepted_candidates<G>(mine, seen, n_seen, seen_ids, I, seed, t, K, lane, iw);
  // ---- score a_1 .. a_cnt, a chunk of rows in flight at a time
  constexpr int C = dynamic_inflight_rows(E);
  ScoredPick s = {WARP ? -1 : 0, 0, 0.f, 0.f, 0.f, 0.f, -1, 0.f};
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] = 0.f;
  int32_t tag_pos = -1;
  float bound = 0.f;  // x_i - margin
  bool found = false;
  if constexpr (WARP) {  // (1) the positive's row, its loads ahead of the first chunk's
#pragma unroll
    for (int e = 0; e < E; ++e) qi[e] = 0.f;
    tag_pos = rows.load(qi, s.bias_pos, pos, gl);
  }
  for (int base = 0; base < K; base += C) {
    // (2) the early stop: a NEG_WARP group with its violator scores no more candidates
    const bool more = WARP ? !found && base < cnt : base < cnt;
    if (!__any(more)) break;
    float row[C][E], bias[C];
    int32_t item[C], tag[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      item[c] = group_bcast<G>(mine, (base + c) & (G - 1), lane);
      bias[c] = 0.f;
      tag[c] = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) row[c][e] = 0.f;
      if (WARP ? more && base + c < cnt : base + c < cnt) tag[c] = rows.load(row[c], bias[c], item[c], gl);
    }
    if constexpr (WARP) {
      if (base == 0) {
        rows.finish(qi, tag_pos, gl);
        s.x_pos = group_sum<G>(dot<E>(p, qi), lane) + s.bias_pos;
        bound = s.x_pos - margin;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (WARP ? more && base + c < cnt : base + c < cnt) rows.finish(row[c], tag[c], gl);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float x = group_sum<G>(dot<E>(p, row[c]), lane) + bias[c];
      bool take;  // (3) the comparison: the first violator, or the best so far
      if constexpr (WARP) take = more && !found && base + c < cnt && x > bound;
      else take = base + c < cnt && (base + c == 0 || x > s.x_neg || (s.x_neg != s.x_neg && x == x));
      if constexpr (WARP) found = found || take;
      s.item = take ? item[c] : s.item;
      if constexpr (WARP) s.tries = take ? base + c + 1 : s.tries;  // (4) tries
      s.x_neg = take ? x : s.x_neg;
      s.bias_neg = take ? bias[c] : s.bias_neg;
      s.tag = take ? tag[c] : s.tag;
#pragma unroll
      for (int e = 0; e < E; ++e) q[e] = take ? row[c][e] : q[e];
    }
  }
  if constexpr (WARP) {  // (5) the weight
    if (found) s.weight = warp_weight((I - 1) - n_seen, s.tries);
  }
  return s;
}

// the item rows as stored (no hot block: the stand-alone kernel sees the table folded)
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

// ---- the arguments of the stand-alone kernel k_sample_scored (bpr_dynamic.hip): one draw per entry of users
// (NEG_WARP: per (user, positive)), on the tables as they are
struct ScoredArgs {
  const float* P;
  const float* Q;
  const float* bias;  // the ctx's dense item_bias, or NULL
  int64_t I;
  int d;
  const int64_t* indptr;
  const int32_t* indices;
  const int32_t* users;
  int64_t n;
  uint64_t seed, offset;
  int32_t K;          // candidates (NEG_DYNAMIC) / max_sampled (NEG_WARP)
  float margin;       // NEG_WARP
  int32_t* neg;
  float* x_neg;       // the pick's score, or NULL
  ItemWeights iw;
};
// NEG_WARP's kernel takes these behind the common arguments (each kind's kernel arguments keep their size)
struct ScoredWarpArgs : ScoredArgs {
  const int32_t* pos;
  int32_t* tries;
  float* x_pos;  // or NULL
};

}  // namespace bpr
