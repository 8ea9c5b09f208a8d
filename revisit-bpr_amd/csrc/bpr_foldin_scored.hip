// bpr_foldin_scored.hip — fold new users in with SCORED negatives (bpr_fold_in_rows_scored): dynamic negatives
// (BPR_NEG_DYNAMIC: the hardest of M unseen candidates under BPR's loss) or the WARP objective (BPR_NEG_WARP: the first
// violator of N, the step weighted by log of the rank estimate), against the frozen item table.  The draw is
// sample_scored (bpr_scored.h) — the device function of k_stream's scored branch and of bpr_sample_dynamic /
// bpr_sample_warp — on the user's row AS IT IS just before the triple's update, with the frozen table behind a
// bounds-checked TableRows.
//
// Shape of the problem: that of k_foldin_adaptive (bpr_foldin_adaptive.hip).  A scored draw depends on the live row,
// so the draw of triple t + 1 comes after the update of triple t, and only the model-independent half of a triple can
// run ahead.  One group of G lanes owns one row at a time (rows by atomic ticket: FOLDIN_NEXT_ROWS,
// bpr_foldin_shared.h; the row in registers from its first triple to its last, no atomics on it) and keeps a ring of PF
// static slots with, per triple fetched ahead, the positive's id and — BPR_NEG_DYNAMIC — its row q_i and bias b_i.  A
// step of the ring, slot s:
//   consume  the triple fetched PF steps ago:  sample_scored(p, ...) -> foldin_update / foldin_update_warp
//   fetch    the row's next triple into slot s (if it has one left)
// A row enters at slot 0, fills the ring in its first PF steps and leaves after total + PF steps.  The triples of a
// row are consumed in triple order by one group and each sees the row as the previous one left it, so the result does
// not depend on PF, on the grid or on which group takes which row.
//
// q_i under BPR_NEG_WARP.  sample_scored needs x_i before its first comparison and loads q_i itself, through
// Rows::load(pos), with the loads of the first chunk of candidate rows: one round trip, which nothing fetched ahead
// would shorten, since the candidates are not known before the draw.  So for this KIND the ring keeps the positive's
// id only and q_i is the draw's: PF * E VGPRs less than an accessor that hands the ring's row back would hold (and no
// per-element select between two sources).  BPR_NEG_DYNAMIC does not score the positive in the draw: its q_i, b_i
// ride the ring and go to foldin_update as in the other kernels.
//
// states_out (the test hook's) is a NULL-checked pointer, not a template flag: the branch is on a kernel argument,
// uniform over the launch.  It costs 2 VGPRs at the four G = 32, E = 1 instantiations and none at the other twenty,
// no occupancy step anywhere (profiles/foldin_scored_resources.md), and one set of kernels serves the product and the
// tests.
//
// Seen structure (bpr_foldin_scored_plan.h; the predicates and the build: bpr_foldin_seen.h): a per-group I-bit bitmap
// in LDS built ONCE per row, or the row's CSR slice; nth_unseen reads the slice in either case.  A group's bitmap is
// touched by its own lanes only, under the group's own predicate.
//
// Wave-uniform control.  The two groups of a G = 32 wave hold different rows of different lengths, and
// accepted_candidates, sample_scored and group_sum must run with the whole wave active.  So the draw is called under
// `__any(consume)`, a condition the whole wave agrees on, and a group with nothing to draw (ring still filling, row
// finished, group out of tickets) takes a DUMMY draw: an empty seen row and ONE candidate; its pick is discarded.
// Why nothing hangs (the ticket loop and the outer loop: FOLDIN_NEXT_ROWS):
//   accepted_candidates   a for-loop of at most UNIFORM_MAX_CAND / G rounds whatever the lanes see; `__all(cnt >= M)`
//                         is only the early exit.  A dummy draw accepts its first candidate (nothing is seen; with
//                         I == 1 every id is outside [0, I), nothing is accepted, and the rank pick is item 0), so it
//                         never prolongs the real draw next to it.
//   sample_scored         a for-loop over base < K <= 32 in steps of the chunk; `!__any(more)` is only the early exit.
//                         K is 1 in a dummy group and `candidates` in a real one: the dummy group leaves the loop
//                         after the first chunk and the real one goes on alone — every collective inside is the
//                         group's own (DPP sums, shuffles inside the group), and the ballot of `more` counts the lanes
//                         still in the loop.
//   nth_unseen, SeenCsr   binary searches over [0, m).
//   the ring              PF steps per trip of the outer loop, `left` falls by one per step while positive.
//
// Nothing here writes Q or item_bias, and no index becomes an address unchecked: a positive outside [1, I) skips its
// triple (BPR_NEG_WARP: the draw scores row 0 in its place, and its answer is reported but not applied), a pick outside
// [1, I) likewise — item 0, what the draw returns when nothing is unseen, among them —, the accessor loads no row
// whose id is outside [0, I) (a CSR that breaks its contract can make nth_unseen return one), a row_order entry outside
// [0, n) is passed over, and a CSR item outside [0, I) is not entered into the bitmap.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <type_traits>

#include "bpr_device.h"
#include "bpr_foldin_scored_plan.h"
#include "bpr_foldin_seen.h"
#include "bpr_foldin_shared.h"
#include "bpr_host.h"
#include "bpr_scored.h"

namespace bpr {

struct FoldinScoredArgs {
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int64_t* indptr;
  const int32_t* items;
  int64_t n;
  const int32_t* row_order;
  int32_t epochs;
  float lr, au;
  int32_t K;     // candidates (BPR_NEG_DYNAMIC) / max_sampled (BPR_NEG_WARP)
  float margin;  // BPR_NEG_WARP
  int32_t* neg_out;
  int32_t* tries_out;
  float* states_out;  // test hook: [epochs * nnz, d], the row as the draw of triple t saw it; NULL in the product
  uint64_t seed, offset;
  float* P;
  uint32_t* ticket;
  int64_t groups;
  int32_t bm_words;
};

// The frozen table as sample_scored reads it: TableRows, and an id outside [0, I) loads nothing (the row stays zero).
template <int G, int E>
struct FrozenRows {
  TableRows<G, E> table;
  int32_t I;
  __device__ __forceinline__ int32_t load(float (&q)[E], float& b, int32_t item, int gl) const {
    if ((uint32_t)item < (uint32_t)I) return table.load(q, b, item, gl);
    return -1;
  }
  __device__ __forceinline__ void finish(float (&)[E], int32_t, int) const {}
};

extern __shared__ uint4 foldin_scored_smem[];

template <int G, int E, int KIND, bool BM, int PF>
__global__ __launch_bounds__(FOLDIN_BLOCK) void k_foldin_scored(const FoldinScoredArgs a) {
  constexpr bool WARP = KIND == NEG_WARP;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int d = a.d;
  const int32_t I = (int32_t)a.I;
  const int64_t base0 = a.indptr[0];
  const int64_t nnz = a.indptr[a.n] - base0;
  uint32_t* const bm = BM ? reinterpret_cast<uint32_t*>(foldin_scored_smem) + (threadIdx.x / G) * a.bm_words
                          : nullptr;
  const FrozenRows<G, E> rows{TableRows<G, E>{a.Q, a.bias, d}, I};
  const ItemWeights no_weights{nullptr, nullptr};  // a context-free call has none

  FOLDIN_ROW_STATE(G, m, a.groups);  // the row this group holds: m positives, drained in PF steps
  int32_t fc = 0, fe = 0, fj = 0;  // fetch: triples fetched, epoch and position of the next one
  int32_t ce = 0, cj = 0;          // consume: epoch and position of the next one
  float p[E];
#pragma unroll
  for (int e = 0; e < E; ++e) p[e] = 0.f;
  // the ring (static slot numbers throughout: a dynamically indexed ring would live in scratch memory)
  int32_t si[PF];  // positive (0 = its triple is skipped)
  float qi[PF][E], bi[PF];  // BPR_NEG_DYNAMIC: its row and bias
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    si[s] = 0;
    bi[s] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) qi[s][e] = 0.f;
  }

  for (;;) {
    // ---- ring slot 0: groups whose row is done write it back and take the next ticket
    FOLDIN_NEXT_ROWS(
        G, m, a.ticket, a.n, a.row_order, a.indptr, a.epochs, PF, (store_row<G, E>(a.P + row * d, p, d, gl);),
        (fc = fe = fj = ce = cj = 0; load_row<G, E>(p, a.P + row * d, d, gl);
         if constexpr (BM) { if (total > 0) FOLDIN_BUILD_BITMAP(G, bm, a.bm_words, a.items, I); }));
    if (__all(finished)) break;

#pragma unroll
    for (int s = 0; s < PF; ++s) {
      // ---- consume: the triple fetched PF steps ago
      {
        const bool cv = !finished && left > 0 && left <= (int64_t)total;
        if (__any(cv)) {
          // !cv: a dummy draw — empty seen row, one candidate, the pick discarded
          using Seen = typename std::conditional<BM, SeenRowBits, SeenRowCsr>::type;
          Seen seen;
          if constexpr (BM) seen = SeenRowBits{bm, I, cv};
          else seen = SeenRowCsr{SeenCsr{a.items, lo, cv ? lo + m : lo}, I};
          const int64_t t = FOLDIN_TRIPLE(ce, cj);
          if (a.states_out != nullptr && cv) store_row<G, E>(a.states_out + t * d, p, d, gl);
          const int32_t i = si[s];
          float qpos[E], qj[E];
          const ScoredPick pick = sample_scored<G, E, KIND>(qpos, qj, p, rows, i, seen, (int64_t)(cv ? m : 0),
                                                            a.items + lo, a.I, a.seed, a.offset + (uint64_t)t,
                                                            cv ? a.K : 1, a.margin, lane, no_weights);
          const int32_t j = pick.item;
          if (cv && gl == 0) {
            if (a.neg_out != nullptr) a.neg_out[t] = j;
            if (a.tries_out != nullptr) a.tries_out[t] = pick.tries;
          }
          // an id outside [1, I) never becomes an address: the triple is skipped (j = 0: nothing unseen; j = -1:
          // BPR_NEG_WARP found no violator)
          const bool ok = cv && i >= 1 && i < I && j >= 1 && j < I;
          if constexpr (WARP) foldin_update_warp<G, E>(p, qpos, qj, pick.weight, ok, a.lr, a.au);
          else foldin_update<G, E>(p, qi[s], qj, bi[s], pick.bias_neg, ok, a.lr, a.au, lane);
          if (cv && ++cj == m) {
            cj = 0;
            ++ce;
          }
        }
      }
      // ---- fetch: the next triple of the row, if it has one left
      {
        const bool valid = !finished && fc < total;
        int32_t i = 0;
        if (valid) i = a.items[lo + fj];
        i = (i >= 1 && i < I) ? i : 0;
        si[s] = i;
        if (valid) {
          if constexpr (!WARP) {
            if (i != 0) {
              load_row<G, E>(qi[s], a.Q + (uint32_t)i * (uint32_t)d, d, gl);
              bi[s] = a.bias != nullptr ? a.bias[i] : 0.f;
            }
          }
          FOLDIN_ADVANCE(fc, fe, fj, m);
        }
      }
      left -= left > 0 ? 1 : 0;
    }
  }
}

}  // namespace bpr

static int fold_in_rows_scored_impl(const char* who, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                    const int64_t* indptr, const int32_t* items, int64_t n, const int32_t* row_order,
                                    int32_t epochs, float lr, float alpha_user, int32_t kind, int32_t candidates,
                                    float margin, int32_t* neg_out, int32_t* tries_out, uint64_t seed, uint64_t offset,
                                    float* P_new, void* hip_stream, int32_t seen_mode, float* states_out) {
  using namespace bpr;
  const std::string w(who);
  if (int rc = foldin_check_shape(who, n, I, d)) return rc;
  if (epochs < 1) return fail(BPR_ERR_INVALID, w + ": epochs must be at least 1");
  if (!(lr == lr) || !(alpha_user == alpha_user)) return fail(BPR_ERR_INVALID, w + ": lr or alpha_user is NaN");
  if (kind == BPR_NEG_GIVEN || kind == BPR_NEG_UNIFORM)
    return fail(BPR_ERR_UNSUPPORTED, w + ": given and uniform negatives are bpr_fold_in_rows'");
  if (kind == BPR_NEG_ADAPTIVE)
    return fail(BPR_ERR_UNSUPPORTED, w + ": adaptive negatives are bpr_fold_in_rows_adaptive's");
  if (!sampler_scored(kind))
    return fail(BPR_ERR_UNSUPPORTED,
                w + ": kind " + std::to_string(kind) + " is not a scored sampler (BPR_NEG_DYNAMIC, BPR_NEG_WARP); " +
                    "bpr_fold_in_rows and bpr_fold_in_rows_adaptive run the others");
  const bool warp = kind == BPR_NEG_WARP;
  if (!(warp ? warp_max_sampled_ok(candidates) : dynamic_candidates_ok(candidates)))
    return fail(BPR_ERR_INVALID, w + ": candidates must be in [1, 32]");
  if (warp && !warp_margin_ok(margin)) return fail(BPR_ERR_INVALID, w + ": margin must be finite and > 0");
  if (seen_mode < FOLDIN_SEEN_AUTO || seen_mode > FOLDIN_SEEN_BITMAP)
    return fail(BPR_ERR_INVALID, w + ": unknown seen_mode");
  if (n == 0) return BPR_OK;
  if (!Q || !indptr || !items || !P_new) return fail(BPR_ERR_INVALID, w + ": Q, indptr, items or P_new is NULL");

  hipStream_t stream = (hipStream_t)hip_stream;
  int64_t nnz = 0;
  if (int rc = foldin_read_nnz(who, indptr, n, epochs, stream, &nnz)) return rc;
  if (nnz == 0) return BPR_OK;

  uint32_t* ticket = nullptr;
  int cus = FOLDIN_CUS;
  if (int rc = foldin_begin(who, stream, &ticket, &cus)) return rc;
  const FoldinScoredPlan pl = plan_foldin_scored(n, I, d, kind, cus, seen_mode);
  FoldinScoredArgs a = {};
  a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.indptr = indptr; a.items = items; a.n = n; a.row_order = row_order;
  a.epochs = epochs; a.lr = lr; a.au = alpha_user; a.K = candidates; a.margin = warp ? margin : 0.f;
  a.neg_out = neg_out; a.tries_out = tries_out; a.states_out = states_out; a.seed = seed; a.offset = offset;
  a.P = P_new; a.ticket = ticket; a.groups = pl.groups; a.bm_words = pl.bm_words;
  return dispatch_ge(pl.G, pl.E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E, PF = foldin_scored_pf(E);
    const dim3 grid((unsigned)pl.grid), block(FOLDIN_BLOCK);
    const size_t lds = (size_t)pl.lds_bytes;
    if (warp) {
      if (pl.bitmap) hipLaunchKernelGGL((k_foldin_scored<G, E, NEG_WARP, true, PF>), grid, block, lds, stream, a);
      else hipLaunchKernelGGL((k_foldin_scored<G, E, NEG_WARP, false, PF>), grid, block, 0, stream, a);
    } else {
      if (pl.bitmap) hipLaunchKernelGGL((k_foldin_scored<G, E, NEG_DYNAMIC, true, PF>), grid, block, lds, stream, a);
      else hipLaunchKernelGGL((k_foldin_scored<G, E, NEG_DYNAMIC, false, PF>), grid, block, 0, stream, a);
    }
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

extern "C" int bpr_fold_in_rows_scored(const float* Q, const float* item_bias, int64_t I, int32_t d,
                                       const int64_t* indptr, const int32_t* items, int64_t n,
                                       const int32_t* row_order, int32_t epochs, float lr, float alpha_user,
                                       int32_t kind, int32_t candidates, float margin, int32_t* neg_out,
                                       int32_t* tries_out, uint64_t seed, uint64_t offset, float* P_new,
                                       void* hip_stream) {
  return fold_in_rows_scored_impl("bpr_fold_in_rows_scored", Q, item_bias, I, d, indptr, items, n, row_order, epochs,
                                  lr, alpha_user, kind, candidates, margin, neg_out, tries_out, seed, offset, P_new,
                                  hip_stream, bpr::FOLDIN_SEEN_AUTO, nullptr);
}

// Test hooks, not API (tests/test_foldin_scored_cpu.py and revisit_bpr/foldin.py set their signatures).
// bpr_fold_in_rows_scored with the seen structure forced (seen_mode 0 = as planned, 1 = CSR, 2 = bitmap) and, when
// states_out [epochs * nnz, d] is not NULL, the row as the draw of every triple saw it (a skipped triple writes its
// unchanged row too).
extern "C" int bpr_test_fold_in_rows_scored(const float* Q, const float* item_bias, int64_t I, int32_t d,
                                            const int64_t* indptr, const int32_t* items, int64_t n,
                                            const int32_t* row_order, int32_t epochs, float lr, float alpha_user,
                                            int32_t kind, int32_t candidates, float margin, int32_t* neg_out,
                                            int32_t* tries_out, uint64_t seed, uint64_t offset, float* P_new,
                                            void* hip_stream, int32_t seen_mode, float* states_out) {
  return fold_in_rows_scored_impl("bpr_test_fold_in_rows_scored", Q, item_bias, I, d, indptr, items, n, row_order,
                                  epochs, lr, alpha_user, kind, candidates, margin, neg_out, tries_out, seed, offset,
                                  P_new, hip_stream, seen_mode, states_out);
}

// The plan of a shape.  in = {n, I, d, cus (0 = the default), seen_mode, kind}; out = {G, E, block, groups_per_block,
// pf, groups, grid, resident, bitmap, bm_words, lds_bytes, lds_max}.  Needs no GPU.
extern "C" int bpr_test_foldin_scored_plan(const int64_t* in, int64_t* out) {
  using namespace bpr;
  if (int rc = foldin_check_shape("bpr_test_foldin_scored_plan", in[0], in[1], (int32_t)in[2])) return rc;
  if (in[4] < FOLDIN_SEEN_AUTO || in[4] > FOLDIN_SEEN_BITMAP)
    return fail(BPR_ERR_INVALID, "bpr_test_foldin_scored_plan: unknown seen_mode");
  if (!sampler_scored((int)in[5])) return fail(BPR_ERR_UNSUPPORTED, "bpr_test_foldin_scored_plan: not a scored kind");
  const FoldinScoredPlan p = plan_foldin_scored(in[0], in[1], (int)in[2], (int)in[5],
                                                in[3] > 0 ? (int)in[3] : FOLDIN_CUS, (int)in[4]);
  const int64_t v[] = {p.G, p.E, p.block, p.groups_per_block, p.pf, p.groups, p.grid, p.resident,
                       p.bitmap, p.bm_words, p.lds_bytes, FOLDIN_ADAPTIVE_LDS_MAX};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}
