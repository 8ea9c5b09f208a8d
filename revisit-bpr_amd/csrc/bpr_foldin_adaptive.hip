// bpr_foldin_adaptive.hip — fold new users in with ADAPTIVE negatives (bpr_fold_in_rows_adaptive): the update of
// k_foldin (bpr_foldin.hip) against the frozen item table, with the negative of every triple drawn by the adaptive
// sampler (AdaptiveSampler.sample, reference modules/neg_samplers.py:74-124) from the user's row AS IT IS just
// before that triple's update.  Q is frozen, so the snapshot (order, sigma) the caller hands in is never stale.
//
// Shape of the problem.  An adaptive negative depends on the live row, so the draw of triple t + 1 comes after the
// update of triple t: unlike k_foldin, only the model-independent half of a triple can run ahead.  One group of G
// lanes owns one row at a time (rows by atomic ticket: FOLDIN_NEXT_ROWS, bpr_foldin_shared.h, the loop all three
// fold-in kernels share; the row in registers from its first triple to its last) and
// keeps a ring of PF static slots with, per triple fetched ahead: the positive's id, its row q_i and bias b_i, and
// the triple's AdaptiveRandoms (seed, counter and the row's length only).  A step of the ring, slot s:
//   consume  the triple fetched PF steps ago:  sample_adaptive(p, ...) -> load q_j, b_j -> foldin_update
//   fetch    the row's next triple into slot s (if it has one left)
// A row enters at slot 0, fills the ring in its first PF steps (nothing to consume yet) and leaves after
// total + PF steps.  The triples of a row are consumed in triple order by one group and each sees the row as the
// previous one left it, so the result does not depend on PF, on the grid or on which group takes which row.
//
// Seen structure (bpr_foldin_adaptive_plan.h; the predicates and the build: bpr_foldin_seen.h): a per-group I-bit
// bitmap in LDS built ONCE per row (zeroed, the row ORed in, a wave-level sync), or the row's CSR slice.  A group's
// bitmap is touched by its own lanes only: the two groups of a G = 32 wave have disjoint words, and the build runs
// under the group's own predicate, so neither a build nor a walk of one group can race with the other's.  LDS
// operations of one wave execute in program order, which is all the ordering a group needs; the fence + wave
// barrier keep the compiler from reordering them.
//
// Wave-uniform control.  The two groups of a G = 32 wave hold different rows of different lengths, and every
// ballot, scan and broadcast inside sample_adaptive / adaptive_walk / foldin_update must run with the whole wave
// active.  So the sampler is called under `__any(consume)`, a condition the whole wave agrees on, and a group with
// nothing to draw (ring still filling, row finished, group out of tickets, or a row with nothing unseen) takes a
// DUMMY draw: an empty seen row and geometric rank 1.  Why adaptive_walk cannot hang (the ticket loop and the outer
// loop: see FOLDIN_NEXT_ROWS): its for-loop is bounded by `base < I` whatever the lanes see, so it ends after at
// most ceil(I / 4G) trips; `__all(done)` is only the early exit.  A dummy draw skips 0 unseen entries of an empty
// seen row, so it is done in the first trip that holds a non-pad entry and never prolongs the real draw next to it
// by more than that.  A real draw's rank is below the row's unseen count, so it is done inside the column.  With
// I == 1 nobody has anything unseen and sample_adaptive walks nothing, uniformly.
//
// Nothing here writes Q, item_bias, order or sigma, and no index becomes an address unchecked: a positive outside
// [1, I) skips its triple, a drawn item outside [1, I) likewise, a row_order entry outside [0, n) is passed over,
// an order entry outside [0, I) is treated as item 0 (never a candidate, never a bitmap index), and a CSR item
// outside [0, I) is not entered into the bitmap.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <type_traits>

#include "bpr_device.h"
#include "bpr_foldin_adaptive_plan.h"
#include "bpr_foldin_seen.h"
#include "bpr_foldin_shared.h"
#include "bpr_host.h"

namespace bpr {

struct FoldinAdaptiveArgs {
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int32_t* order;
  const float* sigma;
  const int64_t* indptr;
  const int32_t* items;
  int64_t n;
  const int32_t* row_order;
  int32_t epochs;
  float lr, au, inv_log1mp;
  int32_t* neg_out;
  int32_t* factor_out;
  int32_t* rank_out;
  uint64_t seed, offset;
  float* P;
  uint32_t* ticket;
  int64_t groups;
  int32_t bm_words;
};

extern __shared__ uint4 foldin_adaptive_smem[];

template <int G, int E, bool BM, int PF>
__global__ __launch_bounds__(FOLDIN_BLOCK) void k_foldin_adaptive(const FoldinAdaptiveArgs a) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int d = a.d;
  const int32_t I = (int32_t)a.I;
  const int64_t base0 = a.indptr[0];
  const int64_t nnz = a.indptr[a.n] - base0;
  uint32_t* const bm = BM ? reinterpret_cast<uint32_t*>(foldin_adaptive_smem) + (threadIdx.x / G) * a.bm_words
                          : nullptr;

  float sg[E];  // the snapshot's sigma, in the row layout
  load_row<G, E>(sg, a.sigma, d, gl);

  FOLDIN_ROW_STATE(G, m, a.groups);  // the row this group holds: m positives, drained in PF steps
  int32_t fc = 0, fe = 0, fj = 0;  // fetch: triples fetched, epoch and position of the next one
  int32_t ce = 0, cj = 0;          // consume: epoch and position of the next one
  float p[E];
#pragma unroll
  for (int e = 0; e < E; ++e) p[e] = 0.f;
  // the ring (static slot numbers throughout: a dynamically indexed ring would live in scratch memory)
  int32_t si[PF];  // positive (0 = its triple is skipped)
  int32_t sr[PF];  // geometric rank of the triple's randoms
  float su[PF];    // their factor uniform
  float qi[PF][E], bi[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    si[s] = 0;
    sr[s] = 1;
    su[s] = bi[s] = 0.f;
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

    const int32_t n_unseen = (I - 1) - m;  // of the row held (m <= I - 1 for a CSR that keeps its contract)
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      // ---- consume: the triple fetched PF steps ago
      {
        const bool cv = !finished && left > 0 && left <= (int64_t)total;
        if (__any(cv)) {
          const bool real = cv && n_unseen > 0;  // else a dummy draw: empty seen row, rank 1
          using Seen = typename std::conditional<BM, SeenRowBits, SeenRowCsr>::type;
          Seen seen;
          if constexpr (BM) seen = SeenRowBits{bm, I, real};
          else seen = SeenRowCsr{SeenCsr{a.items, lo, real ? lo + m : lo}, I};
          AdaptiveRandoms rnd;
          rnd.uf = su[s];
          rnd.r = real ? sr[s] : 1;
          const AdaptiveDraw dr =
              sample_adaptive<G, E, Seen>(p, d, sg, a.order, a.I, seen, (int64_t)(real ? m : 0), rnd, lane);
          const int32_t i = si[s];
          const int32_t j = real ? dr.item : 0;
          if (cv && gl == 0) {
            const int64_t t = FOLDIN_TRIPLE(ce, cj);
            if (a.neg_out != nullptr) a.neg_out[t] = j;
            if (a.factor_out != nullptr) a.factor_out[t] = dr.factor;
            // (a row with nothing unseen: the rank sample_adaptive reports for r = 0)
            if (a.rank_out != nullptr) a.rank_out[t] = real ? dr.rank : (dr.from_top ? -1 : n_unseen);
          }
          // an id outside [1, I) never becomes an address: the triple is skipped
          const bool ok = cv && i >= 1 && i < I && j >= 1 && j < I;
          float qj[E], bj = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) qj[e] = 0.f;
          if (ok) {
            load_row<G, E>(qj, a.Q + (uint32_t)j * (uint32_t)d, d, gl);
            if (a.bias != nullptr) bj = a.bias[j];
          }
          foldin_update<G, E>(p, qi[s], qj, bi[s], bj, ok, a.lr, a.au, lane);
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
          const int64_t t = FOLDIN_TRIPLE(fe, fj);
          const AdaptiveRandoms rnd = adaptive_randoms(a.seed, a.offset + (uint64_t)t, a.inv_log1mp, (int64_t)n_unseen);
          su[s] = rnd.uf;
          sr[s] = rnd.r;
          if (i != 0) {
            load_row<G, E>(qi[s], a.Q + (uint32_t)i * (uint32_t)d, d, gl);
            bi[s] = a.bias != nullptr ? a.bias[i] : 0.f;
          }
          FOLDIN_ADVANCE(fc, fe, fj, m);
        }
      }
      left -= left > 0 ? 1 : 0;
    }
  }
}

}  // namespace bpr

static int fold_in_rows_adaptive_impl(const char* who, const float* Q, const float* item_bias, int64_t I, int32_t d,
                                      const int32_t* order, const float* sigma, const int64_t* indptr,
                                      const int32_t* items, int64_t n, const int32_t* row_order, int32_t epochs,
                                      float lr, float alpha_user, float p, int32_t* neg_out, int32_t* factor_out,
                                      int32_t* rank_out, uint64_t seed, uint64_t offset, float* P_new,
                                      void* hip_stream, int32_t seen_mode) {
  using namespace bpr;
  const std::string w(who);
  if (int rc = foldin_check_shape(who, n, I, d)) return rc;
  if (epochs < 1) return fail(BPR_ERR_INVALID, w + ": epochs must be at least 1");
  if (!(lr == lr) || !(alpha_user == alpha_user)) return fail(BPR_ERR_INVALID, w + ": lr or alpha_user is NaN");
  if (!(p > 0.f && p < 1.f)) return fail(BPR_ERR_INVALID, w + ": p not in (0,1)");
  if (I - 1 > (int64_t)1 << 30)
    return fail(BPR_ERR_UNSUPPORTED, w + ": item ids must not exceed 2^30 (I - 1 <= 2^30: the top bit of an order entry is a flag)");
  if (seen_mode < FOLDIN_SEEN_AUTO || seen_mode > FOLDIN_SEEN_BITMAP)
    return fail(BPR_ERR_INVALID, w + ": unknown seen_mode");
  if (n == 0) return BPR_OK;
  if (!Q || !indptr || !items || !P_new) return fail(BPR_ERR_INVALID, w + ": Q, indptr, items or P_new is NULL");
  if (!order || !sigma) return fail(BPR_ERR_INVALID, w + ": snapshot order or sigma is NULL");

  hipStream_t stream = (hipStream_t)hip_stream;
  int64_t nnz = 0;
  if (int rc = foldin_read_nnz(who, indptr, n, epochs, stream, &nnz)) return rc;
  if (nnz == 0) return BPR_OK;

  uint32_t* ticket = nullptr;
  int cus = FOLDIN_CUS;
  if (int rc = foldin_begin(who, stream, &ticket, &cus)) return rc;
  const FoldinAdaptivePlan pl = plan_foldin_adaptive(n, I, d, cus, seen_mode);
  FoldinAdaptiveArgs a = {};
  a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.order = order; a.sigma = sigma; a.indptr = indptr; a.items = items;
  a.n = n; a.row_order = row_order; a.epochs = epochs; a.lr = lr; a.au = alpha_user; a.inv_log1mp = inv_log1mp(p);
  a.neg_out = neg_out; a.factor_out = factor_out; a.rank_out = rank_out; a.seed = seed; a.offset = offset;
  a.P = P_new; a.ticket = ticket; a.groups = pl.groups; a.bm_words = pl.bm_words;
  return dispatch_ge(pl.G, pl.E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E, PF = foldin_adaptive_pf(E);
    if (pl.bitmap)
      hipLaunchKernelGGL((k_foldin_adaptive<G, E, true, PF>), dim3((unsigned)pl.grid), dim3(FOLDIN_BLOCK),
                         (size_t)pl.lds_bytes, stream, a);
    else
      hipLaunchKernelGGL((k_foldin_adaptive<G, E, false, PF>), dim3((unsigned)pl.grid), dim3(FOLDIN_BLOCK), 0, stream,
                         a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

extern "C" int bpr_fold_in_rows_adaptive(const float* Q, const float* item_bias, int64_t I, int32_t d,
                                         const int32_t* order, const float* sigma, const int64_t* indptr,
                                         const int32_t* items, int64_t n, const int32_t* row_order, int32_t epochs,
                                         float lr, float alpha_user, float p, int32_t* neg_out, int32_t* factor_out,
                                         int32_t* rank_out, uint64_t seed, uint64_t offset, float* P_new,
                                         void* hip_stream) {
  return fold_in_rows_adaptive_impl("bpr_fold_in_rows_adaptive", Q, item_bias, I, d, order, sigma, indptr, items, n,
                                    row_order, epochs, lr, alpha_user, p, neg_out, factor_out, rank_out, seed, offset,
                                    P_new, hip_stream, bpr::FOLDIN_SEEN_AUTO);
}

// Test hooks, not API (tests/test_foldin_adaptive_cpu.py and revisit_bpr/foldin.py set their signatures).
// bpr_fold_in_rows_adaptive with the seen structure forced: seen_mode 0 = as planned, 1 = CSR, 2 = bitmap.
extern "C" int bpr_test_fold_in_rows_adaptive(const float* Q, const float* item_bias, int64_t I, int32_t d,
                                              const int32_t* order, const float* sigma, const int64_t* indptr,
                                              const int32_t* items, int64_t n, const int32_t* row_order,
                                              int32_t epochs, float lr, float alpha_user, float p, int32_t* neg_out,
                                              int32_t* factor_out, int32_t* rank_out, uint64_t seed, uint64_t offset,
                                              float* P_new, void* hip_stream, int32_t seen_mode) {
  return fold_in_rows_adaptive_impl("bpr_test_fold_in_rows_adaptive", Q, item_bias, I, d, order, sigma, indptr, items,
                                    n, row_order, epochs, lr, alpha_user, p, neg_out, factor_out, rank_out, seed,
                                    offset, P_new, hip_stream, seen_mode);
}

// The plan of a shape.  in = {n, I, d, cus (0 = the default), seen_mode}; out = {G, E, block, groups_per_block, pf,
// groups, grid, resident, bitmap, bm_words, lds_bytes, lds_max}.  Needs no GPU.
extern "C" int bpr_test_foldin_adaptive_plan(const int64_t* in, int64_t* out) {
  using namespace bpr;
  if (int rc = foldin_check_shape("bpr_test_foldin_adaptive_plan", in[0], in[1], (int32_t)in[2])) return rc;
  if (in[4] < FOLDIN_SEEN_AUTO || in[4] > FOLDIN_SEEN_BITMAP)
    return fail(BPR_ERR_INVALID, "bpr_test_foldin_adaptive_plan: unknown seen_mode");
  const FoldinAdaptivePlan p =
      plan_foldin_adaptive(in[0], in[1], (int)in[2], in[3] > 0 ? (int)in[3] : FOLDIN_CUS, (int)in[4]);
  const int64_t v[] = {p.G, p.E, p.block, p.groups_per_block, p.pf, p.groups, p.grid, p.resident,
                       p.bitmap, p.bm_words, p.lds_bytes, FOLDIN_ADAPTIVE_LDS_MAX};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}
