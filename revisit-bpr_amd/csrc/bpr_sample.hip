// bpr_sample.hip — fused scoring + sampling of libbprcore: k unseen items per user drawn WITHOUT replacement from
// softmax(score / T) over the user's eligible items (the Plackett-Luce model), in draw order, with no [n, I] score
// matrix anywhere (bpr_sample_rows / bpr_sample_workspace / bpr_sample_slices).
//
// The Gumbel-top-k identity makes this a top-k problem: key(u, i) = score(u, i) / T + g, g independent Gumbel noise,
// and the k largest keys in descending order ARE a Plackett-Luce sample.  So k_sample is k_topk (bpr_topk.hip: 256
// threads, 64 rows, item tiles of 128 x 32 features through LDS into exact f32 MFMA accumulators, selection steps
// (A) (B) (C) on a buffer of k + 128 candidates per row, item slices and k_topk_merge) with Cand{key, id}; read that
// file's header for the structure.  What is new:
//   - the draw (bpr_sample_shared.h): the noise of (row, item) comes from Philox keyed on (seed, draw_id of the row,
//     item), so a row's result is a pure function of the tables, the user, its draw_id, the seed and T — not of n,
//     of the row's place, of item_slices.  A lane's 16 items of one user are 4 runs of 4 consecutive ids: 4 Philox
//     blocks per user, 8 per lane and tile;
//   - the winners' unperturbed scores: k_sample_finish recomputes them after the sweep (and after the merge) with
//     fma_chain8 in one thread per winner, k_rerank's way: bpr_rerank_rows' cand_scores bits, 64 x k x d fmaf per
//     user tile;
//   - the optional log_z[r] = log sum exp(score_i / T) over the row's eligible items whose score is not NaN, so
//     that a caller can log propensities.  Eligibility of EVERY item is needed here (the selection only tests what
//     beats tau): per tile, thread r walks row r's sorted seen row with a cursor and leaves a 128-bit mask.  Then
//     online: per lane max and rescaled sum over its 16 scores of the tile; the two lane halves by one xor-32
//     butterfly; the four waves' partials and the running value in wave order by thread r, tile after tile.  With
//     slices every slice leaves its (max, sum) in the workspace and k_sample_finish combines them in slice order:
//     log_z's bits may depend on item_slices, and for a fixed slice count on nothing else.  exp and log are the
//     fast intrinsics here: log_z is held to a tolerance, the keys are held to bits.
//     The mask and the partials live in the item staging area, idle between a tile's last MFMA and the next tile's
//     first chunk (two more barriers per tile, only when log_z is wanted): the LDS budget is k_topk's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <cmath>
#include <string>

#include "bpr_item_filter.h"
#include "bpr_sample_plan.h"
#include "bpr_sample_shared.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {

struct SampleArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* users;
  const int64_t* draw_ids;  // [n] or NULL = the user id
  int64_t n;
  const int64_t* indptr;
  const int32_t* indices;
  int k, slices;
  int64_t item_tiles;
  float inv_temp;
  uint64_t seed;
  float* out_keys;     // [n, slices, k]
  int32_t* out_items;  // [n, slices, k]
  float2* out_lz;      // [n, slices] (max, sum), or NULL
};

// (max, sum): sum = sum exp(x - max) over what was seen; nothing seen: (-inf, 0)
__device__ __forceinline__ float2 lse_combine(const float2 a, const float2 b) {
  const float m = fmaxf(a.x, b.x);
  if (m == -INFINITY) return make_float2(-INFINITY, 0.f);
  const float sa = a.x == m ? a.y : a.y * __expf(a.x - m);
  const float sb = b.x == m ? b.y : b.y * __expf(b.x - m);
  return make_float2(m, sa + sb);
}

// VEC: d % 4 == 0 and 16-byte aligned tables (16-byte global loads); else element loads.
// FILT: an item filter (bpr_item_filter.h) lies behind the arguments: an item whose bit is clear is not eligible, and
// the loop walks the slice's non-empty tiles only.  Without it the kernel is what it was before there were filters.
// log_z is then the normaliser over the eligible items: the same bit gates its mask.
template <bool VEC, bool FILT>
__global__ __launch_bounds__(256) void k_sample(const MaybeFiltered<FILT, SampleArgs> a) {
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
  // log_z's scratch, over sQ (bpr_sample_plan.h)
  uint32_t* const sMask = reinterpret_cast<uint32_t*>(smem);             // [TU][TI / 32]
  float2* const sPart = reinterpret_cast<float2*>(sMask + TU * TI / 32);  // [4][TU]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t u0 = (int64_t)blockIdx.x * TU;
  const int slice = blockIdx.y;
  const int64_t t0 = a.item_tiles * slice / a.slices, t1 = a.item_tiles * (slice + 1) / a.slices;
  const bool want_lz = a.out_lz != nullptr;

  if (tid < TU) {
    BPR_STAGE_USER_ROW(u0 + tid, a.n, a.users, a.indptr, a.indices, sUser, sSeenLo, sSeenLen);
    BPR_OPEN_SELECTION_ROW(live, sCnt, sNeed, sTau);
  }
  __syncthreads();

  // the lane's two rows' draw ids
  uint64_t did0 = 0, did1 = 0;
  {
    const int64_t row0 = u0 + r, row1 = u0 + 32 + r;
    if (row0 < a.n) did0 = a.draw_ids != nullptr ? (uint64_t)a.draw_ids[row0] : (uint64_t)(int64_t)sUser[r];
    if (row1 < a.n) did1 = a.draw_ids != nullptr ? (uint64_t)a.draw_ids[row1] : (uint64_t)(int64_t)sUser[32 + r];
  }
  // thread r < TU walks row r's seen row for log_z: the cursor starts at the slice's first item
  int seen_cur = 0;
  float2 lz_run = make_float2(-INFINITY, 0.f);
  if (want_lz && tid < TU) {
    const int32_t* const seen = a.indices + sSeenLo[tid];
    int lo = 0, hi = sSeenLen[tid];
    const int64_t first = t0 * TI;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (seen[mid] < first) lo = mid + 1; else hi = mid;
    }
    seen_cur = lo;
  }

  // the walk (bpr_topk_shared.h).  FILT: the slice's non-empty tiles only.
  auto tile_from = [&](int64_t t) -> int64_t {
    if constexpr (FILT) return filter_next_tile(a.filter, a.I, t, t1);
    else return t;
  };
  const table_tiles items = {a.I};
  BPR_WALK_LANE(a.d, sQ, sP);
  BPR_WALK_TILES_BEGIN(VEC, FILT, tile_from(t0), t1, items, a.Q, a.P, a.d, sUser, sQ, sP, tile_from, walk_nop(),
                       walk_nop())

    // ---- log_z: the tile's seen masks, once every wave is done with the staged operands
    if (want_lz) {
      __syncthreads();
      if (tid < TU) {
        const int32_t* const seen = a.indices + sSeenLo[tid];
        const int len = sSeenLen[tid];
        const int64_t lo = t * TI, hi = lo + TI;
        uint32_t bits[TI / 32] = {0u, 0u, 0u, 0u};
        while (seen_cur < len) {
          const int64_t v = seen[seen_cur];
          if (v >= hi) break;
          if (v >= lo) {
            const int b = (int)(v - lo);
#pragma unroll
            for (int j = 0; j < TI / 32; ++j) bits[j] |= (b >> 5) == j ? 1u << (b & 31) : 0u;
          }
          ++seen_cur;
        }
#pragma unroll
        for (int j = 0; j < TI / 32; ++j) sMask[tid * (TI / 32) + j] = bits[j];
      }
      __syncthreads();
    }

    // ---- epilogue of the item tile: register q of the lane is item ibase + (q & 3) + 8 (q >> 2) of users r, 32 + r
    const int64_t ibase = t * TI + 32 * w + 4 * h;
    const bool has_bias = a.bias != nullptr;
    // the wave's word of the filter: bit j is item t * TI + 32 w + j
    uint32_t fw = 0;
    if constexpr (FILT) fw = filter_wave_word(a.filter, a.I, t, __builtin_amdgcn_readfirstlane(w));
    // scores -> keys, in place; log_z's per-lane (max, sum) of the tile on the way
    {
      float x0[16], x1[16];  // score * inv_temp (log_z only)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t first = ibase + 8 * j;  // a multiple of 4: one Philox block per user serves the run
        const u32x4 b0 = sample_block(a.seed, did0, (uint32_t)(first >> 2));
        const u32x4 b1 = sample_block(a.seed, did1, (uint32_t)(first >> 2));
        const uint32_t w0[4] = {b0.x, b0.y, b0.z, b0.w}, w1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = 4 * j + e;
          const int64_t item = first + e;
          const float bv = has_bias && item < a.I ? a.bias[item] : 0.f;
          const float s0 = has_bias ? acc0[q] + bv : acc0[q];
          const float s1 = has_bias ? acc1[q] + bv : acc1[q];
          x0[q] = __fmul_rn(s0, a.inv_temp);
          x1[q] = __fmul_rn(s1, a.inv_temp);
          acc0[q] = sample_key(s0, a.inv_temp, w0[e]);
          acc1[q] = sample_key(s1, a.inv_temp, w1[e]);
        }
      }
      if (want_lz) {
        const uint32_t seen0 = sMask[r * (TI / 32) + w], seen1 = sMask[(32 + r) * (TI / 32) + w];
        float m0 = -INFINITY, m1 = -INFINITY;
        unsigned e0 = 0, e1 = 0;  // eligible and not NaN
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int bit = 4 * h + (q & 3) + 8 * (q >> 2);
          const int64_t item = ibase + (q & 3) + 8 * (q >> 2);
          const bool ok = item > 0 && item < a.I && (!FILT || ((fw >> bit) & 1u));
          if (ok && !((seen0 >> bit) & 1u) && x0[q] == x0[q]) { e0 |= 1u << q; m0 = fmaxf(m0, x0[q]); }
          if (ok && !((seen1 >> bit) & 1u) && x1[q] == x1[q]) { e1 |= 1u << q; m1 = fmaxf(m1, x1[q]); }
        }
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          if (((e0 >> q) & 1u) && m0 != -INFINITY) s0 += x0[q] == m0 ? 1.f : __expf(x0[q] - m0);
          if (((e1 >> q) & 1u) && m1 != -INFINITY) s1 += x1[q] == m1 ? 1.f : __expf(x1[q] - m1);
        }
        float2 l0 = make_float2(m0, s0), l1 = make_float2(m1, s1);
        l0 = lse_combine(l0, make_float2(__shfl_xor(l0.x, 32), __shfl_xor(l0.y, 32)));
        l1 = lse_combine(l1, make_float2(__shfl_xor(l1.x, 32), __shfl_xor(l1.y, 32)));
        if (h == 0) {
          sPart[w * TU + r] = l0;
          sPart[w * TU + 32 + r] = l1;
        }
      }
    }
    // (A) how many keys beat the row's threshold
    unsigned m0 = 0, m1 = 0;
    {
      const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t item = ibase + (q & 3) + 8 * (q >> 2);
        const bool ok = item > 0 && item < a.I && (!FILT || ((fw >> (4 * h + (q & 3) + 8 * (q >> 2))) & 1u));
        if (ok && better(acc0[q], (int)item, tau0.s, tau0.i)) m0 |= 1u << q;
        if (ok && better(acc1[q], (int)item, tau1.s, tau1.i)) m1 |= 1u << q;
      }
      if (m0) atomicAdd(&sNeed[r], __popc(m0));
      if (m1) atomicAdd(&sNeed[32 + r], __popc(m1));
    }
    __syncthreads();
    // (B) rows whose buffer might not take them all are compacted, which tightens tau
    compact_overflowing_rows(sBuf, sCnt, sNeed, sTau, cap, a.k, w, lane);
    // log_z: the four waves' partials onto the row's running value, in wave order
    if (want_lz && tid < TU) {
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) lz_run = lse_combine(lz_run, sPart[ww * TU + tid]);
    }
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
          if (better(acc0[q], item, tau0.s, tau0.i) && !in_sorted(seen0, len0, item)) {
            const int pos = atomicAdd(&sCnt[r], 1);
            if (pos < cap) sBuf[r * cap + pos] = Cand{acc0[q], item};
          }
        }
        if ((m1 >> q) & 1u) {
          if (better(acc1[q], item, tau1.s, tau1.i) && !in_sorted(seen1, len1, item)) {
            const int pos = atomicAdd(&sCnt[32 + r], 1);
            if (pos < cap) sBuf[(32 + r) * cap + pos] = Cand{acc1[q], item};
          }
        }
      }
    }
  BPR_WALK_TILES_END
  __syncthreads();

  if (want_lz && tid < TU && u0 + tid < a.n) a.out_lz[(u0 + tid) * a.slices + slice] = lz_run;

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
      a.out_keys[out + j] = e.s;
      a.out_items[out + j] = e.i;
    }
  }
}

struct FinishArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int d;
  const int32_t* users;
  int k, slices;
  const int32_t* items;  // [n, k]
  float* scores;         // [n, k]
  const float2* lz;      // [n, slices] or NULL
  float* log_z;          // [n] or NULL
};

// One workgroup of TOPK_MAX threads per row: thread j scores winner j — bpr_rerank_rows' cand_scores bits: the chain
// in one thread, every chunk run to its end over zeros past d, then the bias as one fp32 add — and thread 0 combines
// the slices' (max, sum) in slice order into log_z = max + log(sum).
template <bool VEC>
__global__ __launch_bounds__(TOPK_MAX) void k_sample_finish(const FinishArgs a) {
  const int64_t row = blockIdx.x;
  const int j = threadIdx.x;
  if (j < a.k) {
    const int item = a.items[row * a.k + j];
    float s = -INFINITY;
    if (item >= 0) {
      const float* const p = a.P + (int64_t)a.users[row] * a.d;
      const float* const q = a.Q + (int64_t)item * a.d;
      const int dpad = (a.d + TOPK_KC - 1) / TOPK_KC * TOPK_KC;
      float acc = 0.f;
      for (int kk = 0; kk < dpad; kk += 8)
        acc = fma_chain8(load4<VEC>(q, kk, a.d), load4<VEC>(q, kk + 4, a.d), load4<VEC>(p, kk, a.d),
                         load4<VEC>(p, kk + 4, a.d), acc);
      s = a.bias != nullptr ? acc + a.bias[item] : acc;
    }
    a.scores[row * a.k + j] = s;
  }
  if (j == 0 && a.log_z != nullptr) {
    float2 run = make_float2(-INFINITY, 0.f);
    for (int s = 0; s < a.slices; ++s) run = lse_combine(run, a.lz[row * a.slices + s]);
    a.log_z[row] = run.y > 0.f ? run.x + __logf(run.y) : run.x;
  }
}

}  // namespace bpr

extern "C" int bpr_sample_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices,
                                    int32_t want_log_z, int64_t* bytes_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_sample_workspace", bytes_host, "bytes_host")) return rc;
  if (int rc = check_topk_shape("bpr_sample_workspace", n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  *bytes_host = sample_workspace_bytes(n, I, k, item_slices, want_log_z != 0);
  return BPR_OK;
}

extern "C" int bpr_sample_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices,
                                 int32_t* slices_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_sample_slices", slices_host, "slices_host")) return rc;
  if (int rc = check_topk_shape("bpr_sample_slices", n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  *slices_host = plan_topk(n, I, k, item_slices).slices;
  return BPR_OK;
}

namespace bpr {
namespace {

// bpr_sample_rows (rows = "_rows", no filter) and bpr_sample_rows_filtered (rows = "_rows_filtered"): one body, the
// messages under the entry point's own name.  The plan does not look at the filter.
int sample_rows(const char* rows, const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                const int32_t* users, int64_t n, const int64_t* draw_ids, const int64_t* seen_indptr,
                const int32_t* seen_indices, const uint32_t* item_filter, int32_t k, float temperature, uint64_t seed,
                int32_t item_slices, void* workspace, int64_t workspace_bytes, int32_t* items_out, float* scores_out,
                float* keys_out, float* log_z_out, void* hip_stream) {
  const std::string who = std::string("bpr_sample") + rows;
  if (int rc = check_topk_shape(who.c_str(), n, I, d, k, TOPK_MAX, item_slices, "I")) return rc;
  const float inv_temp = 1.0f / temperature;
  if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(inv_temp))
    return fail(BPR_ERR_INVALID, who + ": temperature must be finite and > 0, and so must 1 / temperature");
  if (n > 0 && (!P || !Q || !users || !items_out || !scores_out))
    return fail(BPR_ERR_INVALID, who + ": P, Q, users, items_out or scores_out is NULL");
  if (int rc = check_item_filter(who.c_str(), item_filter)) return rc;
  const bool want_lz = log_z_out != nullptr;
  const SamplePlan p = plan_sample(n, I, k, item_slices, want_lz);
  if (int rc = check_workspace("bpr_sample", workspace, workspace_bytes, p.ws_bytes, "the workspace", false, rows))
    return rc;
  if (n == 0) return BPR_OK;

  hipStream_t stream = (hipStream_t)hip_stream;
  const int S = p.topk.slices;
  // the keys of the result: the caller's buffer, or scores_out until k_sample_finish writes the scores over them
  float* const keys = keys_out != nullptr ? keys_out : scores_out;
  float2* lz = want_lz ? reinterpret_cast<float2*>(reinterpret_cast<unsigned char*>(workspace) + p.topk.ws_bytes)
                       : nullptr;
  SampleArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.users = users; a.draw_ids = draw_ids; a.n = n;
  a.indptr = seen_indptr; a.indices = seen_indices; a.k = k; a.slices = S; a.item_tiles = p.topk.item_tiles;
  a.inv_temp = inv_temp; a.seed = seed;
  slice_outputs(workspace, n, S, k, keys, items_out, &a.out_keys, &a.out_items);
  a.out_lz = lz;
  FinishArgs f = {};
  f.P = P; f.Q = Q; f.bias = item_bias; f.d = d; f.users = users; f.k = k; f.slices = S; f.items = items_out;
  f.scores = scores_out; f.lz = lz; f.log_z = log_z_out;
  const bool vec = vec_path(d, P, Q);
  const dim3 grid((unsigned)p.topk.user_tiles, (unsigned)S);
  if (item_filter != nullptr) {
    Filtered<SampleArgs> fa = {};
    static_cast<SampleArgs&>(fa) = a;
    fa.filter = item_filter;
    if (int rc = launch_kernel(vec ? k_sample<true, true> : k_sample<false, true>, sample_lds_bytes(TOPK_MAX), grid,
                               dim3(256), p.topk.lds, stream, fa))
      return rc;
  } else if (int rc = launch_kernel(vec ? k_sample<true, false> : k_sample<false, false>, sample_lds_bytes(TOPK_MAX),
                                    grid, dim3(256), p.topk.lds, stream, a)) {
    return rc;
  }
  if (int rc = launch_topk_merge(a.out_keys, a.out_items, n, S, k, p.topk.merge_lds, keys, items_out, stream))
    return rc;
  return launch_kernel(vec ? k_sample_finish<true> : k_sample_finish<false>, 0, dim3((unsigned)n), dim3(TOPK_MAX), 0,
                       stream, f);
}

}  // namespace
}  // namespace bpr

extern "C" int bpr_sample_rows(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                               const int32_t* users, int64_t n, const int64_t* draw_ids, const int64_t* seen_indptr,
                               const int32_t* seen_indices, int32_t k, float temperature, uint64_t seed,
                               int32_t item_slices, void* workspace, int64_t workspace_bytes, int32_t* items_out,
                               float* scores_out, float* keys_out, float* log_z_out, void* hip_stream) {
  return bpr::sample_rows("_rows", P, Q, item_bias, I, d, users, n, draw_ids, seen_indptr, seen_indices, nullptr, k,
                          temperature, seed, item_slices, workspace, workspace_bytes, items_out, scores_out, keys_out,
                          log_z_out, hip_stream);
}

extern "C" int bpr_sample_rows_filtered(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                        const int32_t* users, int64_t n, const int64_t* draw_ids,
                                        const int64_t* seen_indptr, const int32_t* seen_indices,
                                        const uint32_t* item_filter, int32_t k, float temperature, uint64_t seed,
                                        int32_t item_slices, void* workspace, int64_t workspace_bytes,
                                        int32_t* items_out, float* scores_out, float* keys_out, float* log_z_out,
                                        void* hip_stream) {
  return bpr::sample_rows("_rows_filtered", P, Q, item_bias, I, d, users, n, draw_ids, seen_indptr, seen_indices,
                          item_filter, k, temperature, seed, item_slices, workspace, workspace_bytes, items_out,
                          scores_out, keys_out, log_z_out, hip_stream);
}
