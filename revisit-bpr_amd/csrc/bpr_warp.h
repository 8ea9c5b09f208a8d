// bpr_warp.h — the WARP objective (Weston, Bengio, Usunier: "WSABIE", IJCAI 2011; LightFM's default loss): draw unseen
// items until one violates the margin, estimate the positive's rank from how many draws that took, weight the step
// by log(rank), skip the triple when nothing violates.  ONE device function, sample_warp, used by k_stream's NEG_WARP
// branch (bpr_stream.h) and by the stand-alone kernel (bpr_warp.hip); the numpy model of it is tests/warp_model.py.
// DESIGN.md §4.17 states the draw.
//
//   candidates   sample_dynamic's (bpr_dynamic.h accepted_candidates): a_1 .. a_m, the first min(N, accepted) unseen
//                candidates of sample_uniform's stream in order, duplicates kept; none accepted: the exact rank pick
//   scores       x_i = <p_u, q_i> (+ b_i), x_k = <p_u, q_{a_k}> (+ b_{a_k}) on the rows the caller's accessor returns
//   violator     the smallest k with x_k > x_i - margin (a NaN on either side compares false); tries = k
//   none         the triple is SKIPPED: item -1, tries 0
//   weight       L = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - |seen(u)|
//
// N = 1 on a user whose every unseen item violates is sample_uniform.
#pragma once
#include "bpr_dynamic.h"

namespace bpr {

struct WarpPick {
  int32_t item;   // the violator, -1 = the triple is skipped
  int32_t tries;  // k of the violator, 0 = skipped
  float x_pos;    // x_i as the kernel computed it
  float x_neg;    // x_k of the violator (0 when skipped)
  float bias_pos, bias_neg;  // the two bias terms (0 without a bias)
  int32_t tag;    // what the accessor's load returned for the violator (k_stream: its hot slot, -1 = none)
  float weight;   // L (0 when skipped)
};

__device__ __forceinline__ float warp_weight(int64_t n_unseen, int tries) {
  const int64_t r = n_unseen / (int64_t)tries;
  return logf((float)(r > 1 ? r : 1));
}

// Rows: as sample_dynamic's.  p[] = the caller's register copy of the user row; qi[] receives the positive's row and
// q[] the violator's (finish() applied to both), so the caller loads neither again.  The rows are loaded a chunk of
// dynamic_inflight<E>() at a time, all of a chunk's loads issued before the first reduction — q_i's with the first
// chunk, x_i has to be known before the first comparison —, and no chunk past the one with the violator is loaded.
// All lanes of the wave must call this together (wave-uniform loops): the groups of a wave walk their chunks in
// lockstep until each has its violator or has run out of candidates.
template <int G, int E, typename Seen, typename Rows>
__device__ __forceinline__ WarpPick sample_warp(float (&qi)[E], float (&q)[E], const float (&p)[E], const Rows& rows,
                                                int32_t pos, const Seen& seen, int64_t n_seen,
                                                const int32_t* __restrict__ seen_ids, int64_t I, uint64_t seed,
                                                uint64_t t, int N, float margin, int lane, const ItemWeights& iw) {
  const int gl = lane & (G - 1);
  int32_t mine;
  const int cnt = accepted_candidates<G>(mine, seen, n_seen, seen_ids, I, seed, t, N, lane, iw);
  constexpr int C = dynamic_inflight<E>();
  WarpPick w = {-1, 0, 0.f, 0.f, 0.f, 0.f, -1, 0.f};
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] = qi[e] = 0.f;
  const int32_t tag_pos = rows.load(qi, w.bias_pos, pos, gl);
  float bound = 0.f;  // x_i - margin
  bool found = false;
  for (int base = 0; base < N; base += C) {
    const bool more = !found && base < cnt;  // this group still looks for its violator
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
      if (more && base + c < cnt) tag[c] = rows.load(row[c], bias[c], item[c], gl);
    }
    if (base == 0) {
      rows.finish(qi, tag_pos, gl);
      w.x_pos = group_sum<G>(dot<E>(p, qi), lane) + w.bias_pos;
      bound = w.x_pos - margin;
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (more && base + c < cnt) rows.finish(row[c], tag[c], gl);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float s = group_sum<G>(dot<E>(p, row[c]), lane) + bias[c];
      const bool take = more && !found && base + c < cnt && s > bound;
      found = found || take;
      w.item = take ? item[c] : w.item;
      w.tries = take ? base + c + 1 : w.tries;
      w.x_neg = take ? s : w.x_neg;
      w.bias_neg = take ? bias[c] : w.bias_neg;
      w.tag = take ? tag[c] : w.tag;
#pragma unroll
      for (int e = 0; e < E; ++e) q[e] = take ? row[c][e] : q[e];
    }
  }
  if (found) w.weight = warp_weight((I - 1) - n_seen, w.tries);
  return w;
}

}  // namespace bpr
