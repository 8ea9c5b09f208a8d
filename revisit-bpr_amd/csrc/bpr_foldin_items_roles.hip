// bpr_foldin_items_roles.hip — item fold-in in BOTH roles (bpr_fold_in_item_rows_roles): the new item is the positive
// of its audience's triples, as in bpr_fold_in_item_rows (bpr_foldin_items.hip), and it is also the NEGATIVE of R
// training interactions (u, i) per epoch of users outside its audience — the triples that would have drawn it in
// joint training with uniform negatives.  Without the second role a folded-in item is only ever pushed up
// ("Cold-start quality").
//
// The kernel is k_foldin_items with one more kind of step in the same four rings of PF register slots; the file
// comment of bpr_foldin_items.hip describes the pipeline, this one what the second role adds.  A row of L users takes
// epochs passes of L + R steps; which of them are negative-role steps is a pure function of (L, R, s) (bprcore.h), and
// the ids stage walks it with a Bresenham accumulator (acc = s R mod (L + R): step s is a negative-role step iff
// acc + R >= L + R) instead of two 64-bit divisions per step.  Nothing on a negative-role step's chain depends on the
// row being learnt either:
//   ids      lane a < 16 of the group draws attempt a: one Philox word -> tau_a -> the loads of train_users[tau_a],
//            train_items[tau_a] are issued (16 attempts in flight at once, none waited for)
//   bounds   each of the 16 lanes tests its own attempt — ids in range, user not in the row's audience: a binary
//            search in the row's own CSR slice, whose bounds (lo, len) are in registers — one ballot picks the first
//            accepted attempt, role_out is written, the load of p_u is issued
//   sample   nothing to draw: the loads of q_i, b_i are issued (the step's `i` takes the place of a given negative)
//   update   x = <p_u, q_i - q> (+ b_i - b), w = sigma(-x), q -= lr (w p_u + alpha q), b -= lr w
// The searches run synchronously inside `bounds`, as the sampler's do inside `sample`; the slice is contiguous and hot
// in cache.  A group whose slot holds the other role's step runs the cross-lane parts (the ballot and the picks here,
// the sampler's there) on a neutral input: no attempt accepted / an empty row.  Control flow around every cross-lane
// step is wave-uniform (__any), as FOLDIN_NEXT_ROWS requires.
//
// With R = 0 every step is a positive-role step and the arithmetic on q, b is k_foldin_items', operation for
// operation: the entry returns bpr_fold_in_item_rows' bits (tests/test_gpu_foldin_items_roles.py).
//
// Nothing here writes P, Q, item_bias, the CSRs or the training arrays (all const); no index can take a load outside
// a table: tau < T by construction, and a training entry out of range is an attempt that is not accepted.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "bpr_device.h"
#include "bpr_foldin_plan.h"
#include "bpr_foldin_shared.h"
#include "bpr_host.h"

namespace bpr {

constexpr uint32_t PURPOSE_ROLE = 2u;  // Philox counter word 3: neither sampler's stream (bpr_device.h: 0 and 1)
constexpr int ROLE_ATTEMPTS = 16;      // attempt a: word a & 3 of block a >> 2

struct FoldinRolesArgs {
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
  const int32_t* train_users;
  const int32_t* train_items;
  uint32_t T;
  int32_t R;
  int32_t* role_out;
};

// One step on the row (q, b) a group holds in registers, in either role, where `upd`:
//   positive role (foldin_item_update's operations, in its order):
//     x = <p_u, q - q_o> + (b - b_o),  w = sigma(-x),  q <- q - lr (-w p_u + alpha_item q),  b <- b + lr w
//   negative role (`neg`; o = the training interaction's item):
//     x = <p_u, q_o - q> + (b_o - b),  w = sigma(-x),  q <- q - lr (w p_u + alpha_item q),   b <- b - lr w
// The dot is an fmaf chain over the lane's elements, then the group's DPP sum.  Wave-uniform call (group_sum).
template <int G, int E>
__device__ __forceinline__ void foldin_item_update_role(float (&q)[E], float& b, const float (&pu)[E],
                                                        const float (&qo)[E], float bo, bool upd, bool neg, bool has_b,
                                                        float lr, float ai, int lane) {
  float xl = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) xl = fmaf(pu[e], neg ? qo[e] - q[e] : q[e] - qo[e], xl);
  float x = group_sum<G>(xl, lane);
  x += neg ? bo - b : b - bo;
  const float w = 1.0f / (1.0f + expf(x));
  const float c = neg ? w : -w;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float qe = q[e];
    const float dq = -lr * (c * pu[e] + ai * qe);
    q[e] = upd ? qe + dq : qe;
  }
  const float lw = lr * w;
  b = (upd && has_b) ? (neg ? b - lw : b + lw) : b;
}

constexpr int32_t NO_TRIPLE = -2, BAD_USER = -1;  // what a ring's user slot holds besides a user id in [0, U)

template <int G, int E, bool SAMPLED, int PF>
__global__ __launch_bounds__(FOLDIN_BLOCK) void k_foldin_items_roles(const FoldinRolesArgs a) {
  static_assert(G >= ROLE_ATTEMPTS, "one lane per attempt");
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int d = a.d;
  const int32_t I = (int32_t)a.I, U = (int32_t)a.U;
  const uint32_t R = (uint32_t)a.R;
  const int64_t base0 = a.indptr[0];
  const int64_t nnz = a.indptr[a.m] - base0;
  FOLDIN_ROW_STATE(G, len, a.groups);  // the row this group holds: len users, len + R steps a pass (`total`: steps)
  // ids stage: steps fetched, epoch, positive-role position k and negative-role count rho of the next step of the
  // pass, and acc = s R mod (len + R)
  int32_t fc = 0, fe = 0, fk = 0, fr = 0;
  uint32_t facc = 0;
  float q[E], b = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) q[e] = 0.f;
  // the rings (static slot numbers throughout: a dynamically indexed ring would live in scratch memory)
  int32_t fu[PF], fx[PF];            // ids: positive role: user (or NO_TRIPLE / BAD_USER); given negative or triple index
                                     //      negative role, PER LANE: the attempt's user and item (loads in flight)
  int32_t ft[PF], fg[PF];            //      negative role: the attempt's tau (per lane); the step's g (-1: positive role)
  int32_t bu[PF], bx[PF];            // bounds: user; given negative / triple index / the accepted interaction's item
  bool bk[PF];                       //         the step's role (true: negative)
  int64_t slo[PF], shi[PF];          //         u's slice of the seen CSR (loads in flight)
  float pa[PF][E];                   //         p_u (loads in flight)
  int32_t un[PF];                    // sample: the other item, whose row is in flight (0 = skip)
  bool uk[PF];                       //         the step's role
  float pu[PF][E], qo[PF][E], bo[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    fu[s] = bu[s] = NO_TRIPLE;
    fx[s] = bx[s] = un[s] = ft[s] = 0;
    fg[s] = -1;
    bk[s] = uk[s] = false;
    slo[s] = shi[s] = 0;
    bo[s] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) pa[s][e] = pu[s][e] = qo[s][e] = 0.f;
  }

  for (;;) {
    // ---- ring slot 0: groups whose row is done write it back and take the next ticket.  (The skeleton counts a
    // row's triples as epochs * len; this kernel's rows take epochs * (len + R) steps, below 2^31 by the host's check,
    // so LOAD sets `total` and `left` again.)
    FOLDIN_NEXT_ROWS(G, len, a.ticket, a.m, a.order, a.indptr, a.epochs, 3 * PF,
                     (store_row<G, E>(a.Qn + row * d, q, d, gl); if (a.bn != nullptr && gl == 0) a.bn[row] = b;),
                     (total = a.epochs * (len + (int32_t)R); left = total > 0 ? (int64_t)total + 3 * PF : 0;
                      fc = fe = fk = fr = 0; facc = 0u; load_row<G, E>(q, a.Qn + row * d, d, gl);
                      b = a.bn != nullptr ? a.bn[row] : 0.f;));
    if (__all(finished)) break;

#pragma unroll
    for (int s = 0; s < PF; ++s) {
      // ---- update: the step whose other row was issued PF steps ago
      foldin_item_update_role<G, E>(q, b, pu[s], qo[s], bo[s], un[s] != 0, uk[s], a.bn != nullptr, a.lr, a.ai, lane);
      // ---- sample: the step whose p_u was issued PF steps ago
      {
        const int32_t u = bu[s];
        const bool role = bk[s];
        int32_t j = 0;
        if constexpr (SAMPLED) {
          const int64_t s_lo = slo[s];
          const int64_t ns = (u >= 0 && !role && shi[s] > s_lo) ? shi[s] - s_lo : 0;
          const bool draw_one = u >= 0 && !role && ns < (int64_t)I - 1;  // a user who has seen every item: 0
          if (__any(draw_one)) {
            // (wave-uniform call: a group with nothing to draw searches an empty row and accepts its first candidate)
            const int64_t n1 = draw_one ? ns : 0;
            const int32_t js = sample_uniform<G>(SeenCsr{a.seen_indices, s_lo, s_lo + n1}, n1, a.seen_indices + s_lo,
                                                 a.I, a.seed, a.offset + (uint64_t)(uint32_t)bx[s], lane);
            j = draw_one ? js : 0;
          }
          if (u != NO_TRIPLE && !role && gl == 0 && a.neg_out != nullptr) a.neg_out[bx[s]] = j;
          j = role ? bx[s] : j;
        } else {
          j = bx[s];  // checked at `ids` (given negative) or at `bounds` (negative role)
        }
        j = u >= 0 ? j : 0;
        un[s] = j;
        uk[s] = role;
#pragma unroll
        for (int e = 0; e < E; ++e) pu[s][e] = pa[s][e];
        if (j != 0) {
          load_row<G, E>(qo[s], a.Q + (uint32_t)j * (uint32_t)d, d, gl);
          bo[s] = a.bias != nullptr ? a.bias[j] : 0.f;
        }
      }
      // ---- bounds: the step fetched PF steps ago.  Negative role: accept an attempt; both: issue the loads
      {
        const int32_t g = fg[s];
        const bool role = g >= 0;
        int32_t u = fu[s], x = fx[s];
        if (__any(role)) {
          // (wave-uniform: a group whose slot holds a positive-role step accepts nothing and ignores the picks)
          bool ok = role && gl < ROLE_ATTEMPTS && u >= 0 && u < U && x >= 1 && x < I;
          if (ok) ok = !csr_contains(a.users, lo, lo + len, u);
          const Ballot acc = wave_ballot(ok);
          const bool any_ok = group_first<G>(acc, lane) >= 0;
          const int32_t pu_ = group_pick<G>(acc, u, lane), px = group_pick<G>(acc, x, lane);
          const int32_t pt = group_pick<G>(acc, ft[s], lane);
          if (role) {
            u = any_ok ? pu_ : BAD_USER;
            x = any_ok ? px : 0;
            if (gl == 0 && a.role_out != nullptr) a.role_out[g] = any_ok ? pt : -1;
          }
        }
        bu[s] = u;
        bx[s] = x;
        bk[s] = role;
        if (u >= 0) {
          if constexpr (SAMPLED) {
            if (!role && a.seen_indptr != nullptr) {
              slo[s] = a.seen_indptr[u];
              shi[s] = a.seen_indptr[u + 1];
            }
          }
          load_row<G, E>(pa[s], a.P + (uint32_t)u * (uint32_t)d, d, gl);
        }
      }
      // ---- ids: the next step of the row, if it has one left
      {
        const bool valid = !finished && fc < total;
        const uint32_t n = (uint32_t)len + R;         // steps of a pass (< 2^31)
        const bool role = valid && facc + R >= n;     // floor((s + 1) R / n) > floor(s R / n)
        const bool posv = valid && !role;
        const int64_t t = FOLDIN_TRIPLE(fe, fk);  // < epochs * nnz < 2^31
        int32_t u = 0, x = 0, tau = 0, g = -1;
        if (posv) u = a.users[lo + fk];
        // an id outside its table never becomes an address: the step is skipped
        bool ok = posv && u >= 0 && u < U;
        if constexpr (SAMPLED) {
          x = (int32_t)t;
        } else {
          if (posv) x = a.neg_in[t];
          ok = ok && x >= 1 && x < I;
          x = ok ? x : 0;
        }
        u = ok ? u : (valid ? BAD_USER : NO_TRIPLE);
        if (role) {
          const int64_t g64 = ((int64_t)fe * a.m + row) * (int64_t)R + fr;  // < epochs * m * R < 2^31
          g = (int32_t)g64;
          u = BAD_USER;
          x = 0;
          if (gl < ROLE_ATTEMPTS) {
            const uint32_t w = draw(a.seed, a.offset + (uint64_t)g64, (uint32_t)gl >> 2, PURPOSE_ROLE, gl & 3);
            tau = (int32_t)__umulhi(w, a.T);  // < T
            u = a.train_users[tau];
            x = a.train_items[tau];
          }
        }
        fu[s] = u;
        fx[s] = x;
        ft[s] = tau;
        fg[s] = g;
        if (valid) {
          ++fc;
          facc += R;
          if (role) {
            facc -= n;
            ++fr;
          } else {
            ++fk;
          }
          if ((uint32_t)fk + (uint32_t)fr == n) {
            fk = fr = 0;
            facc = 0u;
            ++fe;
          }
        }
      }
      left -= left > 0 ? 1 : 0;
    }
  }
}

}  // namespace bpr

extern "C" int bpr_fold_in_item_rows_roles(const float* P, int64_t U, const float* Q, const float* item_bias,
                                           int64_t I, int32_t d, const int64_t* seen_indptr,
                                           const int32_t* seen_indices, const int64_t* indptr, const int32_t* users,
                                           int64_t m, const int32_t* order, int32_t epochs, float lr, float alpha_item,
                                           int32_t sampler, const int32_t* neg_in, int32_t* neg_out, uint64_t seed,
                                           uint64_t offset, const int32_t* train_users, const int32_t* train_items,
                                           int64_t T, int32_t neg_role, int32_t* role_out, float* Q_new,
                                           float* bias_new, void* hip_stream) {
  using namespace bpr;
  const std::string who = "bpr_fold_in_item_rows_roles";
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
  if (neg_role < 0) return fail(BPR_ERR_INVALID, who + ": neg_role must be at least 0");
  if (neg_role > 0) {
    if (!train_users || !train_items)
      return fail(BPR_ERR_INVALID, who + ": neg_role > 0 needs train_users and train_items");
    if (T < 1) return fail(BPR_ERR_INVALID, who + ": neg_role > 0 needs T of at least 1");
    if (T > 0x7FFFFFFF) return fail(BPR_ERR_UNSUPPORTED, who + ": T must be below 2^31");
    if (m > 0 && (int64_t)neg_role > 0x7FFFFFFF / ((int64_t)epochs * m))
      return fail(BPR_ERR_UNSUPPORTED, who + ": epochs * m * neg_role must be below 2^31");
  }
  if (m == 0) return BPR_OK;
  if (!P || !Q || !indptr || !users || !Q_new)
    return fail(BPR_ERR_INVALID, who + ": P, Q, indptr, users or Q_new is NULL");
  if (sampler == BPR_NEG_GIVEN && !neg_in) return fail(BPR_ERR_INVALID, who + ": sampler BPR_NEG_GIVEN needs neg_in");

  hipStream_t stream = (hipStream_t)hip_stream;
  int64_t nnz = 0;
  if (int rc = foldin_read_nnz(who.c_str(), indptr, m, epochs, stream, &nnz)) return rc;
  if (nnz == 0 && neg_role == 0) return BPR_OK;
  // the kernel counts a row's steps, epochs * (L + neg_role), in 32 bits
  if ((int64_t)epochs * (nnz + m * (int64_t)neg_role) > 0x7FFFFFFF)
    return fail(BPR_ERR_UNSUPPORTED, who + ": epochs * (nnz + m * neg_role) must be below 2^31");

  uint32_t* ticket = nullptr;
  int cus = FOLDIN_CUS;
  if (int rc = foldin_begin(who.c_str(), stream, &ticket, &cus)) return rc;
  const FoldinPlan p = plan_foldin(m, d, cus);  // one group per row, rows by ticket: k_foldin's layout
  FoldinRolesArgs a = {};
  a.P = P; a.Q = Q; a.bias = item_bias; a.U = U; a.I = I; a.d = d; a.seen_indptr = seen_indptr;
  a.seen_indices = seen_indices; a.indptr = indptr; a.users = users; a.m = m; a.order = order; a.epochs = epochs;
  a.lr = lr; a.ai = alpha_item; a.neg_in = neg_in; a.neg_out = neg_out; a.seed = seed; a.offset = offset;
  a.Qn = Q_new; a.bn = bias_new; a.ticket = ticket; a.groups = p.groups;
  a.train_users = train_users; a.train_items = train_items; a.T = neg_role > 0 ? (uint32_t)T : 0u; a.R = neg_role;
  a.role_out = role_out;
  const bool sampled = sampler == BPR_NEG_UNIFORM;
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using GEt = decltype(tag);
    constexpr int G = GEt::G, E = GEt::E, PF = foldin_items_pf(E);
    if (sampled)
      hipLaunchKernelGGL((k_foldin_items_roles<G, E, true, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream,
                         a);
    else
      hipLaunchKernelGGL((k_foldin_items_roles<G, E, false, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream,
                         a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}
