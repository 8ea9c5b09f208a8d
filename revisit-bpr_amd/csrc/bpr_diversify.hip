// bpr_diversify.hip — fused diversified top-k of libbprcore: greedy maximal marginal relevance (MMR) over a pool of
// at most 128 candidates per row, with no [n, C, d] gather and no [n, C, C] similarity matrix anywhere
// (bpr_diversify_rows / bpr_diversify_layout; the definition is the comment in include/bprcore.h).
//
// The reference has no such pass: it ranks through full logits (example.py:195-230).  This consumes what
// bpr_topk_rows / bpr_rerank_rows return — [n, C] ids and scores padded with -1 / -inf — and returns the same shape.
//
// One workgroup of 256 threads owns a row (the plan: bpr_diversify_plan.h) and never leaves the CU with it:
//   (E) eligibility, a thread per candidate: 0 < id < I and a finite relevance, BEFORE anything of Q is read; the
//       eligible candidates are compacted in list order (ballot + popcount), E of them, padded to Ep = a multiple of 32;
//   (S) their item rows travel global -> registers -> LDS 32 features at a time in k_topk's padded [rows][32 + 4]
//       chunks, the next chunk in flight while the current one is multiplied;
//   (G) the Ep x Ep Gram matrix is accumulated by v_mfma_f32_32x32x2_f32, the SAME staged chunk on the A and on the
//       B side, in 32 x 32 tiles; only the tiles on or above the diagonal (a wave owns tiles w, w + 4, w + 8 of the
//       at most 10), which then stay in LDS, 33 floats a row.  The diagonal is dot(v, v): the norms come free and
//       are the chain's own bits;
//   (P) the greedy phase, one thread per candidate holding rel', m and a picked flag: each step forms v, reduces the
//       key (v, relevance, -id, -position) to its maximum — shuffles inside the two waves that hold candidates, one
//       LDS exchange between them, ONE barrier a step (the exchange is double-buffered by the step's parity) — and
//       every thread then reads its similarity to the winner: a row of a tile (contiguous) or a column of one
//       (stride 33), 32 lanes on 32 banks either way.
//
// Numerics.  dot(a, b) is k_topk's chain bit for bit (one fp32 accumulator from +0, every chunk of 32 run to its end
// over staged zeros): it IS that MFMA sequence (mfma_block1, bpr_topk_shared.h), with item rows on both sides.
// fp32 multiplication commutes, so G[a][b] and G[b][a] are the same bits and half the matrix suffices.  Cosine is
// dot * (rn(a) * rn(b)) — the product of the two norms first, so that it is symmetric too; rn = 1 / sqrt(dot(v, v)),
// correctly rounded: spelt sqrtf and `/`, with -fhip-fp32-correctly-rounded-divide-sqrt pinned for this object by the
// Makefile (as for bpr_neighbors.hip, whose head says why __fsqrt_rn will not do).  The same flag makes the min-max
// division correctly rounded.  The objective is three separately rounded operations (__fmul_rn, __fmul_rn,
// __fsub_rn; the Makefile's -ffp-contract=off says it again).
//
// Order.  The key's last field is the candidate's position among the row's eligible candidates, which only ever
// separates copies of one (v, relevance, id): the OUTPUT is a function of the multiset of (id, relevance) pairs.
// load4 and the chain are bpr_topk_shared.h's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_diversify_plan.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {
namespace dv {

struct Key {
  float v;      // the objective (a NaN counts, and is reported, as -inf)
  float rel;    // the ORIGINAL relevance
  int32_t id;
  int32_t pos;  // position among the row's eligible candidates; < 0: no candidate
};

struct DivArgs {
  const float* Q;
  int64_t I;
  int d;
  const int32_t* citems;  // [n, C]
  const float* cscores;   // [n, C]
  int64_t n;
  int C, cpad, k;
  float lam, oml;
  int cosine, minmax;
  int32_t* out_items;  // [n, k]
  float* out_scores;   // [n, k]
  float* out_mmr;      // [n, k] or nullptr
};

// larger v, then larger relevance, then smaller id, then smaller position; "no candidate" loses to everything
__device__ __forceinline__ bool better(const Key& a, const Key& b) {
  if (a.pos < 0) return false;
  if (b.pos < 0) return true;
  if (a.v != b.v) return a.v > b.v;
  if (a.rel != b.rel) return a.rel > b.rel;
  if (a.id != b.id) return a.id < b.id;
  return a.pos < b.pos;
}

// VEC: d % 4 == 0 and a 16-byte aligned item table (16-byte global loads); else element loads.
template <bool VEC>
__global__ __launch_bounds__(DIVERSIFY_THREADS) void k_diversify(const DivArgs a) {
  constexpr int KC = DIVERSIFY_KC, LD = DIVERSIFY_LD, TL = DIVERSIFY_TILE, TLD = DIVERSIFY_TILE_LD;
  constexpr int TSZ = TL * TLD;  // floats of a stored Gram tile
  constexpr int NF = DIVERSIFY_CMAX * (KC / 4) / DIVERSIFY_THREADS;  // 16-byte pieces of a chunk a thread moves: 4
  constexpr int NS = 3;  // Gram tiles a wave owns at most: ceil(10 / 4)
  extern __shared__ __align__(16) unsigned char smem[];
  float* const sG = reinterpret_cast<float*>(smem);                    // [tiles][32][33]
  float* const sQ = sG + diversify_tiles(a.cpad) * TSZ;                // [cpad][LD]
  int32_t* const sId = reinterpret_cast<int32_t*>(sQ + a.cpad * LD);   // [cpad], compacted
  float* const sRel = reinterpret_cast<float*>(sId + a.cpad);          // [cpad], compacted
  float* const sRn = sRel + a.cpad;                                    // [cpad]: 1 / norm, < 0: a row with !(ss > 0)
  Key* const sRed = reinterpret_cast<Key*>(sRn + a.cpad);              // [2 parities][2 waves]
  int* const sCnt = reinterpret_cast<int*>(sRed + 4);                  // [2]: eligible candidates of waves 0, 1
  float* const sLoHi = reinterpret_cast<float*>(sCnt + 4);             // [2 waves][lo, hi]

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (a scalar: what depends on it alone is wave-uniform)
  const int nch = (a.d + KC - 1) / KC;

  for (int64_t row = blockIdx.x; row < a.n; row += gridDim.x) {
    // ---- (E) eligibility and compaction, before any row of Q is touched
    int id = -1;
    float rel = 0.f;
    bool ok = false;
    if (tid < a.C) {
      id = a.citems[row * a.C + tid];
      rel = a.cscores[row * a.C + tid];
      ok = id > 0 && id < a.I && __builtin_isfinite(rel);
    }
    const unsigned long long mask = __ballot(ok);
    if (lane == 0 && w < 2) sCnt[w] = __popcll(mask);
    __syncthreads();
    const int E = sCnt[0] + sCnt[1];
    if (ok) {
      const int e = (w == 1 ? sCnt[0] : 0) + __popcll(mask & ((1ull << lane) - 1ull));
      sId[e] = id;
      sRel[e] = rel;
    }
    __syncthreads();
    const int picks = E < a.k ? E : a.k;

    if (picks > 0) {  // (uniform over the workgroup)
      const int Ep = (E + TL - 1) / TL * TL, T = Ep / TL, nt = T * (T + 1) / 2;
      const bool live = tid < E;
      const int myid = live ? sId[tid] : -1;
      const float myrel = live ? sRel[tid] : 0.f;
      if (a.minmax && w < 2) {  // the waves' extremes: read after the barriers of the Gram loop
        float lo = live ? myrel : INFINITY, hi = live ? myrel : -INFINITY;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          lo = fminf(lo, __shfl_xor(lo, off));
          hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if (lane == 0) {
          sLoHi[2 * w] = lo;
          sLoHi[2 * w + 1] = hi;
        }
      }

      // ---- (S) + (G): piece f of a chunk is features 4 (f & 7) .. + 3 of candidate f >> 3
      float4 qreg[NF];
      auto fetch = [&](int c) {
        const int kc = c * KC;
#pragma unroll
        for (int m = 0; m < NF; ++m) {
          const int f = tid + DIVERSIFY_THREADS * m, e = f >> 3;
          qreg[m] = e < E ? load4<VEC>(a.Q + (int64_t)sId[e] * a.d, kc + 4 * (f & 7), a.d)
                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      };
      // the wave's tiles: number w + 4 s of the upper triangle row by row, (ti, tj) with ti <= tj
      int aoff[NS], boff[NS];
      bool own[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        int ti = 0, rem = w + 4 * s;
        own[s] = rem < nt;
        while (own[s] && rem >= T - ti) {
          rem -= T - ti;
          ++ti;
        }
        aoff[s] = own[s] ? (TL * ti + r) * LD + 4 * h : 0;
        boff[s] = own[s] ? (TL * (ti + rem) + r) * LD + 4 * h : 0;
      }
      f32x16 acc[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;

      fetch(0);
      for (int c = 0; c < nch; ++c) {
        __syncthreads();  // the chunk before is read
#pragma unroll
        for (int m = 0; m < NF; ++m) {  // (BPR_STASH_CHUNK's loop, for the tiles the row fills only)
          const int f = tid + DIVERSIFY_THREADS * m;
          if ((f >> 3) < Ep) *reinterpret_cast<float4*>(sQ + (f >> 3) * LD + 4 * (f & 7)) = qreg[m];
        }
        __syncthreads();
        if (c + 1 < nch) fetch(c + 1);
#pragma unroll
        for (int blk = 0; blk < KC / 8; ++blk) {
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            if (!own[s]) continue;  // (wave-uniform)
            const float4 a4 = *reinterpret_cast<const float4*>(sQ + aoff[s] + 8 * blk);
            const float4 b4 = *reinterpret_cast<const float4*>(sQ + boff[s] + 8 * blk);
            mfma_block1(a4, b4, acc[s]);
          }
        }
      }
      // register q of the lane is row (q & 3) + 8 (q >> 2) + 4 h (A side) and column r (B side) of its tile
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (!own[s]) continue;
        float* const g = sG + (w + 4 * s) * TSZ + r;
#pragma unroll
        for (int q = 0; q < 16; ++q) g[((q & 3) + 8 * (q >> 2) + 4 * h) * TLD] = acc[s][q];
      }
      __syncthreads();

      // ---- norms and the scaled relevance (sRn is read after the first step's barrier)
      float myrn = 0.f;
      if (a.cosine && live) {
        const int t = tid >> 5;
        const float ss = sG[(t * T - t * (t - 1) / 2) * TSZ + (tid & 31) * (TLD + 1)];
        myrn = ss > 0.f ? 1.0f / sqrtf(ss) : -1.0f;  // (correctly rounded: the head of this file)
        sRn[tid] = myrn;
      }
      float relp = myrel;
      if (a.minmax) {
        const float lo = fminf(sLoHi[0], sLoHi[2]), hi = fmaxf(sLoHi[1], sLoHi[3]);
        relp = hi == lo ? 0.f : (myrel - lo) / (hi - lo);
      }
      const float lr = __fmul_rn(a.lam, relp);

      // ---- (P) the greedy phase
      float m = 0.f;
      bool picked = false;
      for (int step = 0; step < picks; ++step) {
        Key* const red = sRed + 2 * (step & 1);
        if (w < 2) {
          float v = __fsub_rn(lr, __fmul_rn(a.oml, m));
          if (v != v) v = -INFINITY;
          Key key = {v, myrel, myid, live && !picked ? tid : -1};
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const Key o = {__shfl_xor(key.v, off), __shfl_xor(key.rel, off), __shfl_xor(key.id, off),
                           __shfl_xor(key.pos, off)};
            if (better(o, key)) key = o;
          }
          if (lane == 0) red[w] = key;
        }
        __syncthreads();
        const Key k0 = red[0], k1 = red[1];
        const Key win = better(k1, k0) ? k1 : k0;
        const int p = win.pos;  // >= 0: step < E
        if (tid == 0) {
          a.out_items[row * a.k + step] = win.id;
          a.out_scores[row * a.k + step] = win.rel;
          if (a.out_mmr != nullptr) a.out_mmr[row * a.k + step] = win.v;
        }
        if (tid == p) picked = true;
        if (live) {
          const int tc = tid >> 5, tp = p >> 5;
          float sim = tc <= tp ? sG[(tc * T - tc * (tc - 1) / 2 + tp - tc) * TSZ + (tid & 31) * TLD + (p & 31)]
                               : sG[(tp * T - tp * (tp - 1) / 2 + tc - tp) * TSZ + (p & 31) * TLD + (tid & 31)];
          if (a.cosine) {
            const float rp = sRn[p];
            sim = myrn < 0.f || rp < 0.f ? 0.f : __fmul_rn(sim, __fmul_rn(myrn, rp));
          }
          m = step == 0 || sim > m ? sim : m;
        }
      }
    }

    // ---- the row's tail: fewer than k eligible candidates
    for (int j = picks + tid; j < a.k; j += DIVERSIFY_THREADS) {
      a.out_items[row * a.k + j] = -1;
      a.out_scores[row * a.k + j] = -INFINITY;
      if (a.out_mmr != nullptr) a.out_mmr[row * a.k + j] = -INFINITY;
    }
    __syncthreads();  // the row's LDS is read: the next row may write over it
  }
}

static int check_shape(const char* who, int64_t n, int32_t C, int32_t k, int32_t layout) {
  if (n < 0) return fail(BPR_ERR_INVALID, std::string(who) + ": n must be >= 0");
  if (C < 1 || C > DIVERSIFY_CMAX)
    return fail(BPR_ERR_INVALID, std::string(who) + ": C must be in [1, " + std::to_string(DIVERSIFY_CMAX) + "]");
  if (k < 0 || k > DIVERSIFY_CMAX)
    return fail(BPR_ERR_INVALID, std::string(who) + ": k must be in [0, " + std::to_string(DIVERSIFY_CMAX) + "]");
  if (layout < 0 || layout > DIVERSIFY_LAYOUTS)
    return fail(BPR_ERR_INVALID, std::string(who) + ": layout must be 0 (choose) or 1 (workgroup per row)");
  return BPR_OK;
}

}  // namespace dv
}  // namespace bpr

extern "C" int bpr_diversify_layout(int64_t n, int32_t C, int32_t k, int32_t layout, int32_t* layout_host,
                                    int32_t* cpad_host, int64_t* lds_host) {
  using namespace bpr;
  if (layout_host == nullptr || cpad_host == nullptr || lds_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_diversify_layout: layout_host, cpad_host or lds_host is NULL");
  if (int rc = dv::check_shape("bpr_diversify_layout", n, C, k, layout)) return rc;
  const DiversifyPlan p = plan_diversify(n, C, layout);
  *layout_host = p.layout;
  *cpad_host = p.cpad;
  *lds_host = (int64_t)p.lds;
  return BPR_OK;
}

extern "C" int bpr_diversify_rows(const float* Q, int64_t I, int32_t d, const int32_t* cand_items,
                                  const float* cand_scores, int64_t n, int32_t C, int32_t k, float lam, int32_t metric,
                                  int32_t scale, int32_t layout, int32_t* items_out, float* scores_out, float* mmr_out,
                                  void* hip_stream) {
  using namespace bpr;
  using namespace bpr::dv;
  if (int rc = check_shape("bpr_diversify_rows", n, C, k, layout)) return rc;
  if (d < 1 || d > DIVERSIFY_DMAX) return fail(BPR_ERR_INVALID, "bpr_diversify_rows: d must be in [1, 1024]");
  if (I < 1 || I >= ((int64_t)1 << 31)) return fail(BPR_ERR_INVALID, "bpr_diversify_rows: I must be in [1, 2^31)");
  if (!(lam >= 0.f && lam <= 1.f)) return fail(BPR_ERR_INVALID, "bpr_diversify_rows: lam must be in [0, 1]");
  if (metric != BPR_SIM_DOT && metric != BPR_SIM_COSINE)
    return fail(BPR_ERR_INVALID, "bpr_diversify_rows: metric must be BPR_SIM_DOT or BPR_SIM_COSINE");
  if (scale != BPR_SCALE_NONE && scale != BPR_SCALE_MINMAX)
    return fail(BPR_ERR_INVALID, "bpr_diversify_rows: scale must be BPR_SCALE_NONE or BPR_SCALE_MINMAX");
  if (n == 0 || k == 0) return BPR_OK;
  if (!Q || !cand_items || !cand_scores)
    return fail(BPR_ERR_INVALID, "bpr_diversify_rows: Q, cand_items or cand_scores is NULL");
  if (!items_out || !scores_out) return fail(BPR_ERR_INVALID, "bpr_diversify_rows: items_out or scores_out is NULL");

  const DiversifyPlan p = plan_diversify(n, C, layout);
  DivArgs a = {};
  a.Q = Q; a.I = I; a.d = d; a.citems = cand_items; a.cscores = cand_scores; a.n = n;
  a.C = C; a.cpad = p.cpad; a.k = k; a.lam = lam; a.oml = 1.0f - lam;
  a.cosine = metric == BPR_SIM_COSINE; a.minmax = scale == BPR_SCALE_MINMAX;
  a.out_items = items_out; a.out_scores = scores_out; a.out_mmr = mmr_out;
  hipStream_t stream = (hipStream_t)hip_stream;
  return launch_kernel(vec_path(d, Q) ? k_diversify<true> : k_diversify<false>, 0, dim3((unsigned)p.grid),
                       dim3(DIVERSIFY_THREADS), p.lds, stream, a);
}

// Test hook, not API (tests/test_diversify_cpu.py sets its signature): the plan of a shape.  in = {n, C, k, layout};
// out = {layout, cpad, tiles, grid, lds, lds_limit, grid_max, threads, cmax}.  Needs no GPU.
extern "C" int bpr_test_diversify_plan(const int64_t* in, int64_t* out) {
  using namespace bpr;
  if (int rc = dv::check_shape("bpr_test_diversify_plan", in[0], (int32_t)in[1], (int32_t)in[2], (int32_t)in[3]))
    return rc;
  const DiversifyPlan p = plan_diversify(in[0], (int)in[1], (int)in[3]);
  const int64_t v[] = {p.layout, p.cpad, p.tiles, p.grid, (int64_t)p.lds, (int64_t)DIVERSIFY_LDS_LIMIT,
                       DIVERSIFY_GRID_MAX, DIVERSIFY_THREADS, DIVERSIFY_CMAX};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}
