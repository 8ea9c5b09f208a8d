// bpr_foldin_items.hip — fold new ITEMS into a trained model (bpr_fold_in_item_rows): learn q_i (and b_i) of an item
// that enters the catalogue after training from the list of users who interacted with it, against the FROZEN user
// table, item table and item bias, for a list of items in one launch.
//
// The reference has no such step: its time-split and user-split protocols put every item into the training file.  The
// update is the positive-item half of the sequential BPR step (the q_i and b_i lines of SURVEY §3.3).
//
// Shape of the problem.  This is not k_foldin (bpr_foldin.hip) with its arguments swapped.  A user row reads one seen
// list, its own; an item row meets a different user at every triple, and the negative of triple (u, i_new, j) must be
// unseen by u.  So every triple walks one dependent chain more,
//     users[k] -> seen_indptr[u], seen_indptr[u + 1] -> the sampler's searches in u's CSR row -> q_j, b_j
// beside a gather of p_u from a table of 10^5 rows or more.  Nothing on that chain depends on the row being learnt
// (P, Q, item_bias and the seen CSR do not move; a uniform negative depends on (seed, counter, u's row) only), so all
// of it can run ahead of the one chain that does: dot -> sigma -> axpy on the item row, which lives in registers from
// the first triple to the last.  One group of G lanes (bpr_device.h's layout: G = 32 for d <= 128, else 64) owns one
// new item at a time and runs a four-stage pipeline over the item's triples, one stage per ring of PF register slots:
//   ids      triple c + 3 PF: its user (one index load) and, given negatives, its negative (one more)
//   bounds   triple c + 2 PF: the loads of seen_indptr[u], seen_indptr[u + 1] and of p_u are issued
//   sample   triple c + PF:   the negative is drawn (sample_uniform<G> on u's row), the loads of q_j, b_j are issued
//   update   triple c:        x = <p_u, q - q_j> (+ b - b_j), w = sigma(-x), q -= lr (-w p_u + alpha q), b += lr w
// so no stage waits for a load it has just issued — except inside the sampler: its binary searches in u's row run
// synchronously within `sample`, as in k_foldin (that link is shortened, not hidden).  p_u is issued at `bounds`,
// where its address is first known, and moves from that stage's ring to the update's at `sample`.  A row enters the
// pipeline at ring slot 0 and drains through 3 PF further steps; slots past the row's end carry "no triple".  The
// stages of a triple are the same whatever PF is and the updates of a row are applied in triple order by one group,
// so the result does not depend on PF, on the grid, or on which group takes which row.  PF is BPR_FOLDIN_ITEMS_PF
// (bpr_foldin_plan.h).
//
// Work distribution and wave-uniform control are the shared skeleton's (FOLDIN_NEXT_ROWS, bpr_foldin_shared.h, with
// its whole-wave contract and the argument for its termination): rows by atomic ticket, in the caller's `order` when
// given; the two groups of a G = 32 wave walk different rows in lockstep, every cross-lane step (the DPP sum, the
// sampler's ballots, the ticket broadcast) runs with the whole wave active and per-group predicates, and a group with
// nothing to draw searches an empty row.
//
// Nothing here writes P, Q, item_bias or the seen CSR (all const), there are no atomics on results, and no index can
// take a load outside the tables: a user, a given negative or an `order` entry out of range skips its triple / row.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "bpr_device.h"
#include "bpr_foldin_plan.h"
#include "bpr_foldin_shared.h"
#include "bpr_host.h"

namespace bpr {

struct FoldinItemsArgs {
  const float* P;
  const float* Q;
  const float* bias;
  int64_t U, I;
  int d;
  const int64_t* seen_indptr;
  const int32_t* seen_indices;
  const int64_t* indptr;
  const int32_t* users;
  int64_t m;
  const int32_t* order;
  int32_t epochs;
  float lr, ai;
  const int32_t* neg_in;
  int32_t* neg_out;
  uint64_t seed, offset;
  float* Qn;
  float* bn;
  uint32_t* ticket;
  int64_t groups;
};

// One item fold-in step on the row (q, b) a group holds in registers:
//   x = <p_u, q - q_j> + (b - b_j),  w = sigma(-x),  q <- q - lr (-w p_u + alpha_item q),  b <- b + lr w   where `upd`.
// The dot is an fmaf chain over the lane's elements, then the group's DPP sum, as foldin_update's.  Without a bias
// (`has_b` false) the caller passes b = b_j = 0 and b stays 0.  Wave-uniform call (group_sum).
template <int G, int E>
__device__ __forceinline__ void foldin_item_update(float (&q)[E], float& b, const float (&pu)[E], const float (&qj)[E],
                                                   float bj, bool upd, bool has_b, float lr, float ai,
                                                   int lane) {
  float xl = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) xl = fmaf(pu[e], q[e] - qj[e], xl);
  float x = group_sum<G>(xl, lane);
  x += b - bj;
  const float w = 1.0f / (1.0f + expf(x));
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float qe = q[e];
    const float dq = -lr * (-w * pu[e] + ai * qe);
    q[e] = upd ? qe + dq : qe;
  }
  b = (upd && has_b) ? b + lr * w : b;
}

constexpr int32_t NO_TRIPLE = -2, BAD_USER = -1;  // what a ring's user slot holds besides a user id in [0, U)

template <int G, int E, bool SAMPLED, int PF>
__global__ __launch_bounds__(FOLDIN_BLOCK) void k_foldin_items(const FoldinItemsArgs a) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int d = a.d;
  const int32_t I = (int32_t)a.I, U = (int32_t)a.U;
  const int64_t base0 = a.indptr[0];
  const int64_t nnz = a.indptr[a.m] - base0;
  FOLDIN_ROW_STATE(G, len, a.groups);  // the row this group holds: len users, drained in 3 PF steps
  int32_t fc = 0, fe = 0, fk = 0;  // ids stage: triples fetched, epoch and position of the next one
  float q[E], b = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] = 0.f;
  // the rings (static slot numbers throughout: a dynamically indexed ring would live in scratch memory)
  int32_t fu[PF], fx[PF];            // ids: user (or NO_TRIPLE / BAD_USER); given negative, or triple index (sampled)
  int32_t bu[PF], bx[PF];            // bounds: the same, one stage on
  int64_t slo[PF], shi[PF];          //         u's slice of the seen CSR (loads in flight)
  float pa[PF][E];                   //         p_u (loads in flight)
  int32_t un[PF];                    // sample: the negative whose row is in flight (0 = skip)
  float pu[PF][E], qj[PF][E], bj[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    fu[s] = bu[s] = NO_TRIPLE;
    fx[s] = bx[s] = un[s] = 0;
    slo[s] = shi[s] = 0;
    bj[s] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) pa[s][e] = pu[s][e] = qj[s][e] = 0.f;
  }

  for (;;) {
    // ---- ring slot 0: groups whose row is done write it back and take the next ticket
    FOLDIN_NEXT_ROWS(G, len, a.ticket, a.m, a.order, a.indptr, a.epochs, 3 * PF,
                     (store_row<G, E>(a.Qn + row * d, q, d, gl); if (a.bn != nullptr && gl == 0) a.bn[row] = b;),
                     (fc = fe = fk = 0; load_row<G, E>(q, a.Qn + row * d, d, gl);
                      b = a.bn != nullptr ? a.bn[row] : 0.f;));
    if (__all(finished)) break;

#pragma unroll
    for (int s = 0; s < PF; ++s) {
      // ---- update: the triple whose negative row was issued PF steps ago
      foldin_item_update<G, E>(q, b, pu[s], qj[s], bj[s], un[s] != 0, a.bn != nullptr, a.lr, a.ai, lane);
      // ---- sample: the triple whose bounds and p_u were issued PF steps ago
      {
        const int32_t u = bu[s];
        int32_t j = 0;
        if constexpr (SAMPLED) {
          const int64_t s_lo = slo[s];
          const int64_t ns = (u >= 0 && shi[s] > s_lo) ? shi[s] - s_lo : 0;
          const bool draw_one = u >= 0 && ns < (int64_t)I - 1;  // a user who has seen every item has no negative: 0
          if (__any(draw_one)) {
            // (wave-uniform call: a group with nothing to draw searches an empty row and accepts its first candidate)
            const int64_t n1 = draw_one ? ns : 0;
            const int32_t js = sample_uniform<G>(SeenCsr{a.seen_indices, s_lo, s_lo + n1}, n1, a.seen_indices + s_lo,
                                                 a.I, a.seed, a.offset + (uint64_t)(uint32_t)bx[s], lane);
            j = draw_one ? js : 0;
          }
          if (u != NO_TRIPLE && gl == 0 && a.neg_out != nullptr) a.neg_out[bx[s]] = j;
        } else {
          j = bx[s];  // checked at `ids`
        }
        j = u >= 0 ? j : 0;
        un[s] = j;
#pragma unroll
        for (int e = 0; e < E; ++e) pu[s][e] = pa[s][e];
        if (j != 0) {
          load_row<G, E>(qj[s], a.Q + (uint32_t)j * (uint32_t)d, d, gl);
          bj[s] = a.bias != nullptr ? a.bias[j] : 0.f;
        }
      }
      // ---- bounds: issue the loads of the triple fetched PF steps ago
      {
        const int32_t u = fu[s];
        bu[s] = u;
        bx[s] = fx[s];
        if (u >= 0) {
          if constexpr (SAMPLED) {
            if (a.seen_indptr != nullptr) {
              slo[s] = a.seen_indptr[u];
              shi[s] = a.seen_indptr[u + 1];
            }
          }
          load_row<G, E>(pa[s], a.P + (uint32_t)u * (uint32_t)d, d, gl);
        }
      }
      // ---- ids: the next triple of the row, if it has one left
      {
        const bool valid = !finished && fc < total;
        const int64_t t = FOLDIN_TRIPLE(fe, fk);  // < epochs * nnz < 2^31
        int32_t u = 0, x = 0;
        if (valid) u = a.users[lo + fk];
        // an id outside its table never becomes an address: the triple is skipped
        bool ok = valid && u >= 0 && u < U;
        if constexpr (SAMPLED) {
          x = (int32_t)t;
        } else {
          if (valid) x = a.neg_in[t];
          ok = ok && x >= 1 && x < I;
          x = ok ? x : 0;
        }
        fu[s] = ok ? u : (valid ? BAD_USER : NO_TRIPLE);
        fx[s] = x;
        if (valid) FOLDIN_ADVANCE(fc, fe, fk, len);
      }
      left -= left > 0 ? 1 : 0;
    }
  }
}

}  // namespace bpr

extern "C" int bpr_fold_in_item_rows(const float* P, int64_t U, const float* Q, const float* item_bias, int64_t I,
                                     int32_t d, const int64_t* seen_indptr, const int32_t* seen_indices,
                                     const int64_t* indptr, const int32_t* users, int64_t m, const int32_t* order,
                                     int32_t epochs, float lr, float alpha_item, int32_t sampler,
                                     const int32_t* neg_in, int32_t* neg_out, uint64_t seed, uint64_t offset,
                                     float* Q_new, float* bias_new, void* hip_stream) {
  using namespace bpr;
  const std::string who = "bpr_fold_in_item_rows";
  if (m < 0 || m > 0x7FFFFFFF) return fail(BPR_ERR_INVALID, who + ": m must be in [0, 2^31)");
  if (int rc = foldin_check_shape(who.c_str(), 0, I, d)) return rc;
  if (U < 1) return fail(BPR_ERR_INVALID, who + ": U must be at least 1");
  if (U * (int64_t)d > 0x7FFFFFFF) return fail(BPR_ERR_UNSUPPORTED, who + ": U * d must be below 2^31");
  if (epochs < 1) return fail(BPR_ERR_INVALID, who + ": epochs must be at least 1");
  if (int rc = foldin_check_sampler(who.c_str(), "item fold-in", sampler)) return rc;
  if (!(lr == lr) || !(alpha_item == alpha_item)) return fail(BPR_ERR_INVALID, who + ": lr or alpha_item is NaN");
  if ((item_bias == nullptr) != (bias_new == nullptr))
    return fail(BPR_ERR_INVALID, who + ": item_bias and bias_new must both be given or both be NULL");
  if ((seen_indptr == nullptr) != (seen_indices == nullptr))
    return fail(BPR_ERR_INVALID, who + ": seen_indptr and seen_indices must both be given or both be NULL");
  if (m == 0) return BPR_OK;
  if (!P || !Q || !indptr || !users || !Q_new)
    return fail(BPR_ERR_INVALID, who + ": P, Q, indptr, users or Q_new is NULL");
  if (sampler == BPR_NEG_GIVEN && !neg_in) return fail(BPR_ERR_INVALID, who + ": sampler BPR_NEG_GIVEN needs neg_in");

  hipStream_t stream = (hipStream_t)hip_stream;
  int64_t nnz = 0;
  if (int rc = foldin_read_nnz(who.c_str(), indptr, m, epochs, stream, &nnz)) return rc;
  if (nnz == 0) return BPR_OK;

  uint32_t* ticket = nullptr;
  int cus = FOLDIN_CUS;
  if (int rc = foldin_begin(who.c_str(), stream, &ticket, &cus)) return rc;
  const FoldinPlan p = plan_foldin(m, d, cus);  // one group per row, rows by ticket: k_foldin's layout
  FoldinItemsArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.U = U; a.I = I; a.d = d; a.seen_indptr = seen_indptr;
  a.seen_indices = seen_indices; a.indptr = indptr; a.users = users; a.m = m; a.order = order; a.epochs = epochs;
  a.lr = lr; a.ai = alpha_item; a.neg_in = neg_in; a.neg_out = neg_out; a.seed = seed; a.offset = offset;
  a.Qn = Q_new; a.bn = bias_new; a.ticket = ticket; a.groups = p.groups;
  const bool sampled = sampler == BPR_NEG_UNIFORM;
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E, PF = foldin_items_pf(E);
    if (sampled)
      hipLaunchKernelGGL((k_foldin_items<G, E, true, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream, a);
    else
      hipLaunchKernelGGL((k_foldin_items<G, E, false, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}
