// bpr_hot_kernels.h — the elementwise passes of the item reconciliation and of the hot tier.  None is a template:
// bpr_hot.hip alone includes this header.
#pragma once
#include <stdint.h>

namespace bpr {

// ---------------------------------------------------------------------------------------------
// item-table reconciliation (multi-GPU): the two elementwise passes around the RCCL all-reduce,
// each ONE pass over the table (HBM bound: 12 B / 24 B moved per element)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_item_delta(const float* __restrict__ q,
                                                    const float* __restrict__ base,
                                                    float* __restrict__ own,
                                                    float* __restrict__ tot, int64_t n) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const float dlt = q[k] - base[k];
    own[k] = dlt;
    tot[k] = dlt;
  }
}

__global__ __launch_bounds__(256) void k_item_fold(float* __restrict__ q, float* __restrict__ base,
                                                   const float* __restrict__ own,
                                                   const float* __restrict__ tot, float scale,
                                                   int rebase, int64_t n) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const float st = scale * tot[k];
    const float nb = base[k] + st;  // identical on every rank: the bases never drift apart
    base[k] = nb;
    q[k] = rebase ? nb : q[k] + (st - own[k]);
  }
}

// fold of the previous reconciliation and cut of the next delta in one pass (nothing trained in
// between): q += st - own; base += st; own = tot = q - base
__global__ __launch_bounds__(256) void k_item_fold_delta(float* __restrict__ q,
                                                         float* __restrict__ base,
                                                         float* __restrict__ own,
                                                         float* __restrict__ tot, float scale,
                                                         int64_t n) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const float st = scale * tot[k];
    const float nb = base[k] + st;
    const float nq = q[k] + (st - own[k]);
    const float dl = nq - nb;
    base[k] = nb;
    q[k] = nq;
    own[k] = dl;
    tot[k] = dl;
  }
}

// ---------------------------------------------------------------------------------------------
// two-tier reconciliation, HOT tier (multi-GPU): the hot block of a launch is exchanged on its own,
// every launch (or sub-launch), while the cold rows wait for the per-period all-reduce.
//   hb  [H, d]  the hot rows as of the last reconciled exchange — bit-identical on every rank
//               (only all-reduced sums are ever added to it), canonical row order
//   tot [H, d]  in: the all-reduced sum of every rank's deltas of the PREVIOUS exchange (fold_prev);
//               out: this rank's deltas of the launch just finished (cut), to be all-reduced next
// One pass: hb += tot_prev;  dl = delta[slot] (summed over replicas), delta = 0;  tot = dl;
//           Q[item] = hb + dl   — the reconciled value plus what only this rank knows so far.
// cold_base (optional): the cold tier's base of the same rows is set to the new Q, so that the cold
// tier's delta of a hot row is exactly zero (hot rows travel in the hot tier only).
// ---------------------------------------------------------------------------------------------
struct HotStepArgs {
  float* Q;
  float* delta;
  const int32_t* hot_items;
  const int32_t* canon;
  float* hb;
  float* tot;
  float* cold_base;
  int32_t H, R, d, fold_prev, cut;
};

__global__ __launch_bounds__(256) void k_hot_step(const HotStepArgs a) {
  const int64_t n = (int64_t)a.H * a.d;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(k / a.d), f = (int)(k % a.d);
    const int32_t it = a.hot_items[s];
    const int64_t c = (int64_t)a.canon[s] * a.d + f;
    float b = a.hb[c];
    if (a.fold_prev) b += a.tot[c];
    float dl = 0.f;
    if (a.cut) {
      for (int r = 0; r < a.R; ++r) {
        dl += a.delta[(int64_t)r * n + k];
        a.delta[(int64_t)r * n + k] = 0.f;
      }
      a.tot[c] = dl;
    }
    a.hb[c] = b;
    if (it >= 0) {
      const int64_t q = (int64_t)it * a.d + f;
      a.Q[q] = b + dl;
      if (a.cold_base != nullptr) a.cold_base[q] = b + dl;
    }
  }
}

// hb = the hot rows of Q in canonical order (start of the hot tier: replicas are identical)
__global__ __launch_bounds__(256) void k_hot_gather(const float* __restrict__ Q,
                                                    const int32_t* __restrict__ hot_items,
                                                    const int32_t* __restrict__ canon,
                                                    float* __restrict__ hb, int H, int d) {
  const int64_t n = (int64_t)H * d;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(k / d), f = (int)(k % d);
    hb[(int64_t)canon[s] * d + f] = Q[(int64_t)hot_items[s] * d + f];
  }
}

}  // namespace bpr
