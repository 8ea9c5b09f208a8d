// bpr_foldin.hip — fold new users into a trained model (bpr_fold_in_rows): learn p_u from a new user's history
// against the FROZEN item table (and item bias), for a list of users in one launch.
//
// The reference has no such step: its held-out users' histories are part of the training file
// (full-train-with-fold-in.jsonl), which is why its configs/RQ3/user-split protocol has no BPR entry.  The update is
// the user half of the sequential BPR step (the p_u line of SURVEY §3.3; k_stream applies all three).
//
// Shape of the problem.  Q does not move and a uniform negative depends on (seed, counter, the user's row) only, so
// everything a user's E * m triples will read is known before the first update; the one dependent chain is
// dot -> sigma -> axpy on the user row, which lives in registers from the first triple to the last.  One group of G
// lanes (bpr_device.h's layout: G = 32 for d <= 128, else 64) owns one user at a time and runs a three-stage
// pipeline over the user's triples, one stage per ring of PF register slots:
//   fetch    triple c + 2 PF: its positive (one index load) and its negative (neg_in, or sample_uniform<G>)
//   rows     triple c + PF:   the loads of q_i, q_j (and b_i, b_j) are issued from the indices fetched PF steps ago
//   update   triple c:        x = <p, q_i - q_j> (+ b_i - b_j), w = sigma(-x), p -= lr (-w (q_i - q_j) + alpha p)
// so an update never waits for a load it has just issued.  A row enters the pipeline at ring slot 0 and drains
// through 2 PF further steps; slots past the row's end carry negative 0, which is also what "nothing unseen" gives:
// a triple with negative 0 is skipped.  The stages of a triple are the same whatever PF is and the updates of a row
// are applied in triple order by one group, so the result does not depend on PF, on the grid, or on which group
// takes which row.  PF is BPR_FOLDIN_PF (bpr_foldin_plan.h).
//
// Work distribution.  Row lengths span three orders of magnitude, so groups take rows by an atomic ticket, in the
// caller's `order` (longest first) when given: FOLDIN_NEXT_ROWS (bpr_foldin_shared.h), the loop all three fold-in
// kernels share, with its whole-wave contract and the argument for its termination.  The two groups of a G = 32
// wave walk different rows in lockstep: every cross-lane step (the DPP sum, the sampler's ballots, the ticket
// broadcast) runs with the whole wave active and per-group predicates; a group whose row ends mid-ring idles to
// slot 0.
//
// Nothing here writes Q or item_bias, and no index can take a load outside the tables: a positive, a given negative
// or an `order` entry out of range skips its triple / row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <mutex>
#include <string>

#include "bpr_device.h"
#include "bpr_foldin_plan.h"
#include "bpr_foldin_shared.h"
#include "bpr_host.h"

namespace bpr {

struct FoldinArgs {
  const float* Q;
  const float* bias;
  int64_t I;
  int d;
  const int64_t* indptr;
  const int32_t* items;
  int64_t n;
  const int32_t* order;
  int32_t epochs;
  float lr, au;
  const int32_t* neg_in;
  int32_t* neg_out;
  uint64_t seed, offset;
  float* P;
  uint32_t* ticket;
  int64_t groups;
};

template <int G, int E, bool SAMPLED, int PF>
__global__ __launch_bounds__(FOLDIN_BLOCK) void k_foldin(const FoldinArgs a) {
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1);
  const int d = a.d;
  const int32_t I = (int32_t)a.I;
  const int64_t base0 = a.indptr[0];
  const int64_t nnz = a.indptr[a.n] - base0;
  FOLDIN_ROW_STATE(G, m, a.groups);  // the row this group holds: m positives, drained in 2 PF steps
  int32_t fc = 0, fe = 0, fj = 0;  // fetch stage: triples fetched, epoch and position of the next one
  float p[E];
#pragma unroll
  for (int e = 0; e < E; ++e) p[e] = 0.f;
  // the rings (static slot numbers throughout: a dynamically indexed ring would live in scratch memory)
  int32_t fi[PF], fn[PF];      // fetched: positive, negative (0 = skip)
  int32_t rn[PF];              // rows stage: the negative whose rows are in flight (0 = skip)
  float qi[PF][E], qj[PF][E], bi[PF], bj[PF];
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    fi[s] = fn[s] = rn[s] = 0;
    bi[s] = bj[s] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) qi[s][e] = qj[s][e] = 0.f;
  }

  for (;;) {
    // ---- ring slot 0: groups whose row is done write it back and take the next ticket
    FOLDIN_NEXT_ROWS(G, m, a.ticket, a.n, a.order, a.indptr, a.epochs, 2 * PF,
                     (store_row<G, E>(a.P + row * d, p, d, gl);),
                     (fc = fe = fj = 0; load_row<G, E>(p, a.P + row * d, d, gl);));
    if (__all(finished)) break;

#pragma unroll
    for (int s = 0; s < PF; ++s) {
      // ---- update: the triple whose rows were issued PF steps ago
      foldin_update<G, E>(p, qi[s], qj[s], bi[s], bj[s], rn[s] != 0, a.lr, a.au, lane);
      // ---- rows: issue the loads of the triple fetched PF steps ago
      {
        const int32_t i = fi[s], j = fn[s];
        rn[s] = j;
        if (j != 0) {
          load_row<G, E>(qi[s], a.Q + (uint32_t)i * (uint32_t)d, d, gl);
          load_row<G, E>(qj[s], a.Q + (uint32_t)j * (uint32_t)d, d, gl);
          if (a.bias != nullptr) {
            bi[s] = a.bias[i];
            bj[s] = a.bias[j];
          }
        }
      }
      // ---- fetch: the next triple of the row, if it has one left
      {
        const bool valid = !finished && fc < total;
        const int64_t t = FOLDIN_TRIPLE(fe, fj);
        int32_t i = 0, j = 0;
        if (valid) i = a.items[lo + fj];
        if constexpr (SAMPLED) {
          const bool draw_one = valid && m < I - 1;  // a row that covers every item has no negative: 0
          if (__any(draw_one)) {
            // (wave-uniform call: a group with nothing to draw searches an empty row and accepts its first candidate)
            const int32_t ms = draw_one ? m : 0;
            const int32_t js = sample_uniform<G>(SeenCsr{a.items, lo, lo + ms}, (int64_t)ms, a.items + lo, a.I,
                                                 a.seed, a.offset + (uint64_t)t, lane);
            j = draw_one ? js : 0;
          }
          if (valid && gl == 0 && a.neg_out != nullptr) a.neg_out[t] = j;
        } else {
          if (valid) j = a.neg_in[t];
        }
        // an id outside [1, I) never becomes an address: the triple is skipped
        const bool ok = valid && i >= 1 && i < I && j >= 1 && j < I;
        fi[s] = ok ? i : 0;
        fn[s] = ok ? j : 0;
        if (valid) FOLDIN_ADVANCE(fc, fe, fj, m);
      }
      left -= left > 0 ? 1 : 0;
    }
  }
}

int foldin_check_shape(const char* who, int64_t n, int64_t I, int32_t d) {
  if (n < 0 || n > 0x7FFFFFFF) return fail(BPR_ERR_INVALID, std::string(who) + ": n must be in [0, 2^31)");
  if (d < 1) return fail(BPR_ERR_INVALID, std::string(who) + ": d must be in [1, 1024]");
  if (d > FOLDIN_MAX_D) return fail(BPR_ERR_UNSUPPORTED, std::string(who) + ": d must be in [1, 1024]");
  if (I < 1) return fail(BPR_ERR_INVALID, std::string(who) + ": I must be at least 1");
  if (I * (int64_t)d > 0x7FFFFFFF) return fail(BPR_ERR_UNSUPPORTED, std::string(who) + ": I * d must be below 2^31");
  return BPR_OK;
}

// Ticket words, one 128-byte line each, handed out round-robin: a call zeroes its own in stream order, so calls on
// different streams do not share one (until FOLDIN_TICKETS calls are in flight at once).  Allocated at a device's
// first call and kept for the life of the process.
constexpr int FOLDIN_TICKETS = 256, FOLDIN_TICKET_STRIDE = 32, FOLDIN_MAX_DEV = 64;
static std::mutex g_ticket_mu;
static uint32_t* g_tickets[FOLDIN_MAX_DEV];
static unsigned g_ticket_next[FOLDIN_MAX_DEV];
static int g_cus[FOLDIN_MAX_DEV];

int foldin_check_sampler(const char* who, const char* noun, int32_t sampler) {
  if (sampler == BPR_NEG_ADAPTIVE)
    return fail(BPR_ERR_UNSUPPORTED, std::string(who) + ": adaptive negatives are not implemented for " + noun);
  if (int rc = refuse_scored(std::string(who) + " (" + noun + ")", sampler)) return rc;
  if (sampler != BPR_NEG_GIVEN && sampler != BPR_NEG_UNIFORM)
    return fail(BPR_ERR_INVALID, std::string(who) + ": unknown sampler " + std::to_string(sampler));
  return BPR_OK;
}

int foldin_read_nnz(const char* who, const int64_t* indptr, int64_t rows, int32_t epochs, hipStream_t stream,
                    int64_t* nnz) {
  int64_t ends[2] = {0, 0};
  BPR_HIP_CHECK(hipMemcpyAsync(&ends[0], indptr, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  BPR_HIP_CHECK(hipMemcpyAsync(&ends[1], indptr + rows, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  BPR_HIP_CHECK(hipStreamSynchronize(stream));
  *nnz = ends[1] - ends[0];
  if (ends[0] < 0 || *nnz < 0) return fail(BPR_ERR_INVALID, std::string(who) + ": indptr does not ascend");
  if (*nnz > 0x7FFFFFFF / (int64_t)epochs)
    return fail(BPR_ERR_UNSUPPORTED, std::string(who) + ": epochs * nnz must be below 2^31");
  return BPR_OK;
}

int foldin_next_ticket(const char* who, uint32_t** out, int* cus) {
  int dev = 0;
  BPR_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= FOLDIN_MAX_DEV) return fail(BPR_ERR_UNSUPPORTED, std::string(who) + ": device index too large");
  std::lock_guard<std::mutex> lock(g_ticket_mu);
  if (g_tickets[dev] == nullptr) {
    BPR_HIP_CHECK(hipDeviceGetAttribute(&g_cus[dev], hipDeviceAttributeMultiprocessorCount, dev));
    BPR_HIP_CHECK(hipMalloc(&g_tickets[dev], sizeof(uint32_t) * FOLDIN_TICKETS * FOLDIN_TICKET_STRIDE));
  }
  *out = g_tickets[dev] + (size_t)(g_ticket_next[dev]++ % FOLDIN_TICKETS) * FOLDIN_TICKET_STRIDE;
  *cus = g_cus[dev];
  return BPR_OK;
}

int foldin_begin(const char* who, hipStream_t stream, uint32_t** ticket, int* cus) {
  if (int rc = foldin_next_ticket(who, ticket, cus)) return rc;
  BPR_HIP_CHECK(hipMemsetAsync(*ticket, 0, sizeof(uint32_t), stream));
  return BPR_OK;
}

}  // namespace bpr

extern "C" int bpr_fold_in_rows(const float* Q, const float* item_bias, int64_t I, int32_t d, const int64_t* indptr,
                                const int32_t* items, int64_t n, const int32_t* order, int32_t epochs, float lr,
                                float alpha_user, int32_t sampler, const int32_t* neg_in, int32_t* neg_out,
                                uint64_t seed, uint64_t offset, float* P_new, void* hip_stream) {
  using namespace bpr;
  const char* who = "bpr_fold_in_rows";
  if (int rc = foldin_check_shape(who, n, I, d)) return rc;
  if (epochs < 1) return fail(BPR_ERR_INVALID, "bpr_fold_in_rows: epochs must be at least 1");
  if (int rc = foldin_check_sampler(who, "fold-in", sampler)) return rc;
  if (!(lr == lr) || !(alpha_user == alpha_user))
    return fail(BPR_ERR_INVALID, "bpr_fold_in_rows: lr or alpha_user is NaN");
  if (n == 0) return BPR_OK;
  if (!Q || !indptr || !items || !P_new)
    return fail(BPR_ERR_INVALID, "bpr_fold_in_rows: Q, indptr, items or P_new is NULL");
  if (sampler == BPR_NEG_GIVEN && !neg_in)
    return fail(BPR_ERR_INVALID, "bpr_fold_in_rows: sampler BPR_NEG_GIVEN needs neg_in");

  hipStream_t stream = (hipStream_t)hip_stream;
  int64_t nnz = 0;
  if (int rc = foldin_read_nnz(who, indptr, n, epochs, stream, &nnz)) return rc;
  if (nnz == 0) return BPR_OK;

  uint32_t* ticket = nullptr;
  int cus = FOLDIN_CUS;
  if (int rc = foldin_begin(who, stream, &ticket, &cus)) return rc;
  const FoldinPlan p = plan_foldin(n, d, cus);
  FoldinArgs a = {};
  a.Q = Q; a.bias = item_bias; a.I = I; a.d = d; a.indptr = indptr; a.items = items; a.n = n; a.order = order;
  a.epochs = epochs; a.lr = lr; a.au = alpha_user; a.neg_in = neg_in; a.neg_out = neg_out; a.seed = seed;
  a.offset = offset; a.P = P_new; a.ticket = ticket; a.groups = p.groups;
  const bool sampled = sampler == BPR_NEG_UNIFORM;
  return dispatch_ge(p.G, p.E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E, PF = foldin_pf(E);
    if (sampled)
      hipLaunchKernelGGL((k_foldin<G, E, true, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream, a);
    else
      hipLaunchKernelGGL((k_foldin<G, E, false, PF>), dim3((unsigned)p.grid), dim3(FOLDIN_BLOCK), 0, stream, a);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

// Test hook, not API (tests/test_foldin_cpu.py sets its signature): the plan of a shape.  in = {n, d, cus (0 = the
// default)}; out = {G, E, block, groups_per_block, pf, groups, grid, resident}.  Needs no GPU.
extern "C" int bpr_test_foldin_plan(const int64_t* in, int64_t* out) {
  using namespace bpr;
  if (int rc = foldin_check_shape("bpr_test_foldin_plan", in[0], 1, (int32_t)in[1])) return rc;
  const FoldinPlan p = plan_foldin(in[0], (int)in[1], in[2] > 0 ? (int)in[2] : FOLDIN_CUS);
  const int64_t v[] = {p.G, p.E, p.block, p.groups_per_block, p.pf, p.groups, p.grid, FOLDIN_RESIDENT};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}
