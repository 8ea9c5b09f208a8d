// bpr_retrieve.hip — the deep first stage of libbprcore: the k <= 1,024 best unseen items of a list of users, fused
// scoring + selection with no [n, I] score matrix (bpr_retrieve_rows / bpr_retrieve_workspace / bpr_retrieve_slices).
//
// k_topk (bpr_topk.hip) stops at k = 128 because its 64 rows keep k + 128 candidates each in LDS.  k_retrieve is the
// same tile loop — 64 users x 128 items x 32 features at a time through LDS into exact f32 MFMA accumulators, the
// chain of bpr_topk_shared.h, so a score has bpr_topk_rows' bits — with the rows' candidate buffers in device memory:
// a workgroup owns one block of 64 x cap (score, id) pairs of the workspace (cap: bpr_retrieve_plan.h, a power of two
// >= 2 k), and LDS holds the staged operands, the rows' meta data and a scratch of 4 x cap pairs.
//
// Selection.  Per row: a threshold tau = (score, id) — its k-th best at the last compaction — a count, and `need`.
// After an item tile: (A) every lane counts its scores that beat tau; (B) a row whose buffer might not take them
// (count + need > cap) is compacted by one wave: buffer -> scratch, bitonic sort by `better`, the k best and the new
// tau back; (C) scores that beat the current tau are appended (atomic slot in LDS, the pair to device memory, every
// store behind `pos < cap`).  compact_row's rank by counting is quadratic — no option at 2,048 entries; the network
// is n log^2 n, 64 lanes wide.  `better` is a strict total order on what a buffer holds (ids are distinct), so the
// sorted row does not depend on the order the appends took their slots in: the output is a pure function of the
// inputs.  Seen items: (C) appends WITHOUT looking at the user's seen row; the compaction does, for what was
// appended since the last one (`checked` entries at the front are known to be unseen), every lane its own binary
// search — the tile loop never touches the CSR.  tau is then the k-th best of unseen items only, so it is the bound
// it would be had the seen items never entered, and a seen item costs a slot until the next compaction, no more.
//
// Barriers.  The buffer is device memory written by some lanes of the workgroup and read by others.  (C) of a tile
// and (B) of a later one are separated by the __syncthreads of the chunk loop and the one after (A); (B)'s write-back
// and (C) by the one after (B): __syncthreads orders the workgroup's device-memory accesses as well as its LDS
// accesses (a workgroup's waves share a CU and its vector cache).  Inside a compaction the wave alone touches its
// scratch and its row; the network's stages are separated by wave barriers and wavefront fences.
//
// Persistent grid.  plan_retrieve bounds the workgroups (as many as stay resident, from TOPK_CUS); workgroup b
// walks the (user tile, slice) pairs b, b + grid, ... and reuses its block, so the workspace is grid blocks plus the
// slices' partial results whatever n is.  Item slices, their partial results and the merge are k_topk's
// (launch_topk_merge, bpr_serving_host.h), with slices x k <= 8,192.
//
// Measured (profiles/retrieve_probe.txt, ML-20M shape, d = 128; the composition is P[users] Q^T, the seen scatter and
// torch.topk(k) per 4,096 users).  All 138,493 users: k = 128 31.5 ms against 58.8 (and against k_topk's 99.6: the
// tile loop without the CSR searches is what that kernel's header asks for), k = 256 45.9 against 60.1 — and then it
// LOSES: k = 512 74.4 against 60.4, k = 1,024 204.2 against 61.2.  4,096 users (64 user tiles x 4 slices): it loses
// at every k, 3.1 / 4.8 / 7.5 / 11.4 ms against 1.8 - 1.9.  Suspected reasons, not measured apart: the sort — a
// compaction at cap = 2,048 is 66 stages of 16 LDS compare-exchanges per lane, run by ONE wave while the row's other
// lanes wait at the barrier, and with a random table a row sees about k ln(I / k) candidates after the fill, one
// compaction per cap - k of them and one more at the end; the composition's cost barely moves with k.  At 4,096
// users one workgroup per CU leaves the MFMA pipe idle during every epilogue, the merge is a second launch, and the
// composition is a single GEMM there.  Next steps: sort the small strides in registers (DPP / shuffles) instead of
// through LDS, merge the k sorted survivors with the sorted tail instead of sorting all of it again, and give the
// compaction to all 4 waves of the row's workgroup.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_item_filter.h"
#include "bpr_retrieve_plan.h"
#include "bpr_serving_host.h"
#include "bpr_topk_shared.h"

namespace bpr {

struct RetrieveArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* users;
  int64_t n;
  const int64_t* indptr;
  const int32_t* indices;
  int k, slices, cap;
  int64_t item_tiles, units;
  Cand* bufs;          // [grid][TOPK_TU][cap]
  float* out_scores;   // [n, slices, k]
  int32_t* out_items;  // [n, slices, k]
};

// One wave: the c <= cap candidates of a row in device memory -> scratch (LDS, [cap]), the entries from `checked`
// on that are in the sorted seen row dropped, sorted by `better`.  Returns how many are left; they are scratch[0 ..).
// What is dropped or past c is the sentinel (-inf, INT_MAX), which every candidate beats (ids are below INT_MAX) and
// which therefore sorts last.  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ int sort_row(const Cand* buf, int c, int checked, const int32_t* __restrict__ seen,
                                        int seen_len, Cand* scratch, int lane) {
  int n2 = 64;  // (a power of two >= c, and at least one entry per lane)
  while (n2 < c) n2 <<= 1;
  int dropped = 0;
  for (int idx = lane; idx < n2; idx += 64) {
    Cand e = {-INFINITY, INT_MAX};
    if (idx < c) {
      e = buf[idx];
      if (idx >= checked && in_sorted(seen, seen_len, e.i)) {
        e = Cand{-INFINITY, INT_MAX};
        ++dropped;
      }
    }
    scratch[idx] = e;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dropped += __shfl_xor(dropped, off, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // the bitonic network over n2 entries: pair t of a stage is (i, i + stride), i = t with a 0 bit put in at `stride`
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (n2 >> 1); t += 64) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const Cand x = scratch[i], y = scratch[j];
        const bool first = (i & size) == 0;  // best first in this block of the stage, or best last
        if (first ? better(y.s, y.i, x.s, x.i) : better(x.s, x.i, y.s, y.i)) {
          scratch[i] = y;
          scratch[j] = x;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  return c - dropped;
}

// VEC: d % 4 == 0 and 16-byte aligned tables (16-byte global loads); else element loads.
// FILT: an item filter (bpr_item_filter.h) lies behind the arguments: an item whose bit is clear is not eligible, and
// the loop walks the unit's non-empty tiles only.  Without it the kernel is what it was before there were filters.
template <bool VEC, bool FILT>
__global__ __launch_bounds__(256) void k_retrieve(const MaybeFiltered<FILT, RetrieveArgs> a) {
  constexpr int TU = TOPK_TU, TI = TOPK_TI, LD = TOPK_LD;
  extern __shared__ __align__(16) unsigned char smem[];
  const int cap = a.cap;
  float* const sQ = reinterpret_cast<float*>(smem);               // [TI][LD]
  float* const sP = sQ + TI * LD;                                 // [TU][LD]
  Cand* const sScratch = reinterpret_cast<Cand*>(sP + TU * LD);   // [4][cap]
  Cand* const sTau = sScratch + 4 * cap;                          // [TU]
  int64_t* const sSeenLo = reinterpret_cast<int64_t*>(sTau + TU);
  int* const sCnt = reinterpret_cast<int*>(sSeenLo + TU);
  int* const sNeed = sCnt + TU;
  int* const sUser = sNeed + TU;
  int* const sSeenLen = sUser + TU;
  int* const sChecked = sSeenLen + TU;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  Cand* const gBuf = a.bufs + (int64_t)blockIdx.x * TU * cap;  // this workgroup's block: [TU][cap]
  Cand* const scratch = sScratch + w * cap;
  BPR_WALK_LANE(a.d, sQ, sP);  // (once for all units)
  const bool has_bias = a.bias != nullptr;

  for (int64_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const int64_t u0 = unit / a.slices * TU;
    const int slice = (int)(unit % a.slices);
    const int64_t t0 = a.item_tiles * slice / a.slices, t1 = a.item_tiles * (slice + 1) / a.slices;

    if (tid < TU) {
      BPR_STAGE_USER_ROW(u0 + tid, a.n, a.users, a.indptr, a.indices, sUser, sSeenLo, sSeenLen);
      BPR_OPEN_SELECTION_ROW(live, sCnt, sNeed, sTau, sChecked[tid] = 0);
    }
    __syncthreads();

    // one wave: row's buffer -> its scratch, unseen and sorted; returns how many
    auto sorted_row = [&](int row) {
      return sort_row(gBuf + (int64_t)row * cap, min(sCnt[row], cap), sChecked[row], a.indices + sSeenLo[row],
                      sSeenLen[row], scratch, lane);
    };

    // the walk (bpr_topk_shared.h).  FILT: the unit's non-empty tiles only.
    auto tile_from = [&](int64_t t) -> int64_t {
      if constexpr (FILT) return filter_next_tile(a.filter, a.I, t, t1);
      else return t;
    };
    const table_tiles items = {a.I};
    BPR_WALK_TILES_BEGIN(VEC, FILT, tile_from(t0), t1, items, a.Q, a.P, a.d, sUser, sQ, sP, tile_from, walk_nop(),
                         walk_nop())
      // ---- epilogue of the item tile: register q of the lane is item ibase + (q & 3) + 8 (q >> 2) of users r, 32 + r
      const int64_t ibase = t * TI + 32 * w + 4 * h;
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
      __syncthreads();  // (the appends of the tiles before are behind this barrier too)
      // (B) rows whose buffer might not take them all: down to the k best unseen, which tightens tau
      for (int row = w; row < TU; row += 4) {
        const int c = min(sCnt[row], cap);
        if (c + sNeed[row] <= cap) continue;
        const int left = sorted_row(row);
        const int keep = left < a.k ? left : a.k;
        Cand* const buf = gBuf + (int64_t)row * cap;
        for (int j = lane; j < keep; j += 64) buf[j] = scratch[j];
        if (lane == 0) {
          if (left >= a.k) sTau[row] = scratch[a.k - 1];
          sCnt[row] = keep;
          sChecked[row] = keep;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the scratch is free for the wave's next row)
      }
      __syncthreads();
      // (C) append what still beats the threshold; whether the user has seen it is the compaction's question
      if (tid < TU) sNeed[tid] = 0;
      if (m0 | m1) {
        const Cand tau0 = sTau[r], tau1 = sTau[32 + r];
        Cand* const buf0 = gBuf + (int64_t)r * cap;
        Cand* const buf1 = gBuf + (int64_t)(32 + r) * cap;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int item = (int)(ibase + (q & 3) + 8 * (q >> 2));
          if ((m0 >> q) & 1u) {
            const float s0 = has_bias ? acc0[q] + bv[q] : acc0[q];
            if (better(s0, item, tau0.s, tau0.i)) {
              const int pos = atomicAdd(&sCnt[r], 1);
              if (pos < cap) buf0[pos] = Cand{s0, item};
            }
          }
          if ((m1 >> q) & 1u) {
            const float s1 = has_bias ? acc1[q] + bv[q] : acc1[q];
            if (better(s1, item, tau1.s, tau1.i)) {
              const int pos = atomicAdd(&sCnt[32 + r], 1);
              if (pos < cap) buf1[pos] = Cand{s1, item};
            }
          }
        }
      }
    BPR_WALK_TILES_END
    __syncthreads();

    // ---- the unit's result: every row unseen and sorted, straight from the scratch, padded with (-inf, -1)
    for (int row = w; row < TU; row += 4) {
      if (u0 + row >= a.n) break;
      const int left = sorted_row(row);
      const int have = left < a.k ? left : a.k;
      const int64_t out = ((u0 + row) * a.slices + slice) * a.k;
      for (int j = lane; j < a.k; j += 64) {
        const Cand e = j < have ? scratch[j] : Cand{-INFINITY, -1};
        a.out_scores[out + j] = e.s;
        a.out_items[out + j] = e.i;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();  // (the next unit resets the rows' meta data and reuses the block)
  }
}

}  // namespace bpr

extern "C" int bpr_retrieve_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices,
                                      int64_t* bytes_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_retrieve_workspace", bytes_host, "bytes_host")) return rc;
  if (int rc = check_topk_shape("bpr_retrieve_workspace", n, I, d, k, RETRIEVE_MAX, item_slices, "I")) return rc;
  *bytes_host = retrieve_workspace_bytes(n, I, k, item_slices);
  return BPR_OK;
}

extern "C" int bpr_retrieve_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices,
                                   int32_t* slices_host) {
  using namespace bpr;
  if (int rc = check_out("bpr_retrieve_slices", slices_host, "slices_host")) return rc;
  if (int rc = check_topk_shape("bpr_retrieve_slices", n, I, d, k, RETRIEVE_MAX, item_slices, "I")) return rc;
  *slices_host = plan_retrieve(n, I, k, item_slices).slices;
  return BPR_OK;
}

namespace bpr {
namespace {

// bpr_retrieve_rows (rows = "_rows", no filter) and bpr_retrieve_rows_filtered (rows = "_rows_filtered"): one body,
// the messages under the entry point's own name.  The plan does not look at the filter.
int retrieve_rows(const char* rows, const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                  const int32_t* users, int64_t n, const int64_t* seen_indptr, const int32_t* seen_indices,
                  const uint32_t* item_filter, int32_t k, int32_t item_slices, void* workspace,
                  int64_t workspace_bytes, int32_t* items_out, float* scores_out, void* hip_stream) {
  const std::string who = std::string("bpr_retrieve") + rows;
  if (int rc = check_topk_shape(who.c_str(), n, I, d, k, RETRIEVE_MAX, item_slices, "I")) return rc;
  if (n > 0 && (!P || !Q || !users || !items_out || !scores_out))
    return fail(BPR_ERR_INVALID, who + ": P, Q, users, items_out or scores_out is NULL");
  if (int rc = check_item_filter(who.c_str(), item_filter)) return rc;
  const RetrievePlan p = plan_retrieve(n, I, k, item_slices);
  if (int rc = check_workspace("bpr_retrieve", workspace, workspace_bytes, p.ws_bytes, "workspace", true, rows))
    return rc;
  if (n == 0) return BPR_OK;

  hipStream_t stream = (hipStream_t)hip_stream;
  RetrieveArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.users = users; a.n = n;
  a.indptr = seen_indptr; a.indices = seen_indices; a.k = k; a.slices = p.slices; a.cap = p.cap;
  a.item_tiles = p.item_tiles; a.units = p.units;
  // the rows' candidate buffers lie behind the slices' partial lists
  a.bufs = reinterpret_cast<Cand*>(reinterpret_cast<unsigned char*>(workspace) + p.part_bytes);
  slice_outputs(workspace, n, p.slices, k, scores_out, items_out, &a.out_scores, &a.out_items);
  const bool vec = vec_path(d, P, Q);
  if (item_filter != nullptr) {
    Filtered<RetrieveArgs> f = {};
    static_cast<RetrieveArgs&>(f) = a;
    f.filter = item_filter;
    if (int rc = launch_kernel(vec ? k_retrieve<true, true> : k_retrieve<false, true>,
                               retrieve_lds_bytes(RETRIEVE_MAX), dim3((unsigned)p.grid), dim3(256), p.lds, stream, f))
      return rc;
  } else if (int rc = launch_kernel(vec ? k_retrieve<true, false> : k_retrieve<false, false>,
                                    retrieve_lds_bytes(RETRIEVE_MAX), dim3((unsigned)p.grid), dim3(256), p.lds,
                                    stream, a)) {
    return rc;
  }
  return launch_topk_merge(a.out_scores, a.out_items, n, p.slices, k, p.merge_lds, scores_out, items_out, stream);
}

}  // namespace
}  // namespace bpr

extern "C" int bpr_retrieve_rows(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                 const int32_t* users, int64_t n, const int64_t* seen_indptr,
                                 const int32_t* seen_indices, int32_t k, int32_t item_slices, void* workspace,
                                 int64_t workspace_bytes, int32_t* items_out, float* scores_out, void* hip_stream) {
  return bpr::retrieve_rows("_rows", P, Q, item_bias, I, d, users, n, seen_indptr, seen_indices, nullptr, k,
                            item_slices, workspace, workspace_bytes, items_out, scores_out, hip_stream);
}

extern "C" int bpr_retrieve_rows_filtered(const float* P, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                          const int32_t* users, int64_t n, const int64_t* seen_indptr,
                                          const int32_t* seen_indices, const uint32_t* item_filter, int32_t k,
                                          int32_t item_slices, void* workspace, int64_t workspace_bytes,
                                          int32_t* items_out, float* scores_out, void* hip_stream) {
  return bpr::retrieve_rows("_rows_filtered", P, Q, item_bias, I, d, users, n, seen_indptr, seen_indices, item_filter,
                            k, item_slices, workspace, workspace_bytes, items_out, scores_out, hip_stream);
}

// Test hook, not API (tests/test_retrieve_cpu.py sets its signature): the plan of a shape.  in = {n, I, d, k,
// item_slices, cus}; out = {slices, user_tiles, item_tiles, tile_users, tile_items, cap, lds, merge_lds, ws_bytes,
// units, grid, grid_max, part_bytes, buf_bytes}; bounds[0 .. slices] = first item of each slice, then I.  No GPU.
extern "C" int bpr_test_retrieve_plan(const int64_t* in, int64_t* out, int64_t* bounds) {
  using namespace bpr;
  if (int rc = check_topk_shape("bpr_test_retrieve_plan", in[0], in[1], (int32_t)in[2], (int32_t)in[3], RETRIEVE_MAX,
                                (int32_t)in[4], "I"))
    return rc;
  const int cus = in[5] > 0 ? (int)in[5] : TOPK_CUS;
  const RetrievePlan p = plan_retrieve(in[0], in[1], (int)in[3], (int)in[4], cus);
  const int64_t v[] = {p.slices, p.user_tiles, p.item_tiles, TOPK_TU, TOPK_TI, p.cap, (int64_t)p.lds,
                       (int64_t)p.merge_lds, p.ws_bytes, p.units, p.grid, retrieve_grid_max((int)in[3], cus),
                       p.part_bytes, p.buf_bytes};
  memcpy(out, v, sizeof(v));
  slice_bounds(p, retrieve_slice_tile, TOPK_TI, in[1], bounds);
  return BPR_OK;
}
