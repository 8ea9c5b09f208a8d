// bpr_foldin_shared.h — the skeleton the fold-in kernels are built on (k_foldin, bpr_foldin.hip;
// k_foldin_adaptive, bpr_foldin_adaptive.hip; k_foldin_scored, bpr_foldin_scored.hip; k_foldin_items,
// bpr_foldin_items.hip).  Device side: the row a group holds (FOLDIN_ROW_STATE), the loop in which groups hand rows
// back and take the next by ticket (FOLDIN_NEXT_ROWS), the cursor a pipeline stage walks a row's triples with
// (FOLDIN_TRIPLE, FOLDIN_ADVANCE), and the user-row updates of the three user kernels: foldin_update (BPR's step) and
// its sibling foldin_update_warp (the WARP objective's step, k_foldin_scored alone); the item kernels have an update
// of their own.  Host side: the checks and the launch prologue every fold-in entry point runs (bpr_fold_in_rows,
// _adaptive, _scored, bpr_fold_in_item_rows).  What differs between the kernels, their pipeline stages, stays in
// their files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpr_device.h"
#include "bpr_foldin_plan.h"

// ---- The row-ticket skeleton.  These are macros, not functions: every function form tried (the row as a struct by
// reference or by value, its scalars by reference, the store / load as lambdas, forced inline or not) takes the
// address of state that the kernels otherwise keep in plain locals, the compiler then schedules the kernels
// differently, and three instantiations of k_foldin lose an occupancy step (profiles/foldin_skeleton_resources.md).
// Expanded in place, the code below compiles to the instructions of the loop written out in each kernel.  Being
// macros they have no scope: they are for the kernels of namespace bpr, and they name the kernel's locals — those of
// FOLDIN_ROW_STATE, and `lane`, `gl`, `nnz`, `base0` as every fold-in kernel declares them.

// The row a group owns, the same in every lane of the group: its number (-1: none), where it starts in the CSR,
// its entries LEN and triples `total` (epochs * LEN < 2^31, checked by the host), and `left`, the pipeline steps
// until its last update is applied (total + drain may pass 2^31).  `finished`: the group is out of tickets; a lane
// beyond the launch's groups starts so.
#define FOLDIN_ROW_STATE(LANES, LEN, GROUPS)                                                    \
  bool finished = ((int64_t)blockIdx.x * FOLDIN_BLOCK + threadIdx.x) / (LANES) >= (GROUPS);       \
  int64_t row = -1, lo = 0;                                                                   \
  int32_t LEN = 0, total = 0;                                                                 \
  int64_t left = 0

// Ring slot 0 of every fold-in kernel: each group whose row is done (left == 0) writes it back (STORE) and takes
// tickets until one gives it a row with triples — ORDER[ticket] when ORDER is given; then it sets the row's extent,
// left = total + DRAIN (the extra steps the kernel's pipeline needs to apply the last update) and runs LOAD: read
// the row, reset the kernel's cursors — or until the tickets are past the N rows.  STORE and LOAD are parenthesised
// statement lists, and both name the row `row`.  LANES: the group's width.  The kernel's outer loop ends on
// `__all(finished)` right after it.
//
// Contract: expanded where the WHOLE WAVE is active (the top of the kernel's outer loop, outside any divergent
// branch).  The two groups of a G = 32 wave hold different rows, so the ballots and the broadcast here run on all 64
// lanes under per-group predicates; STORE and LOAD run under the group's own predicate and must not assume the other
// group is with them.
//
// Why it cannot hang.  A group with `need` takes a ticket in every trip of the loop; the ticket either gives it a
// row with triples (left > 0: need drops), or is past the list (finished: need drops), or names an empty or
// out-of-range row, and the next trip takes another ticket.  Tickets only grow and the list is finite, so every
// group reaches `finished` after at most N + groups tickets in all.  `left` falls by one per pipeline step while
// positive, so a group is back here after total + DRAIN steps, rounded up to the kernel's ring.  `__all(finished)`
// is evaluated by the whole wave right after the loop, where no lane is masked off.
#define FOLDIN_STATEMENTS(...) __VA_ARGS__
#define FOLDIN_NEXT_ROWS(LANES, LEN, TICKET, N, ORDER, INDPTR, EPOCHS, DRAIN, STORE, LOAD)        \
  do {                                                                                        \
    bool need = !finished && left == 0;                                                       \
    while (__any(need)) {                                                                     \
      if (need && row >= 0) {                                                                 \
        FOLDIN_STATEMENTS STORE                                                               \
      }                                                                                       \
      uint32_t tk = 0u;                                                                       \
      if (need && gl == 0) tk = atomicAdd(TICKET, 1u);                                        \
      tk = group_bcast<LANES>(tk, 0, lane);                                                   \
      if (need) {                                                                             \
        row = -1;                                                                             \
        LEN = total = 0;                                                                      \
        left = 0;                                                                             \
        if ((int64_t)tk >= (N)) {                                                             \
          finished = true;                                                                    \
        } else {                                                                              \
          const int64_t r = (ORDER) != nullptr ? (int64_t)(ORDER)[tk] : (int64_t)tk;          \
          if (r >= 0 && r < (N)) {                                                            \
            row = r;                                                                          \
            lo = (INDPTR)[r];                                                                 \
            LEN = (int32_t)((INDPTR)[r + 1] - lo);                                            \
            total = (EPOCHS) * LEN;                                                           \
            left = total > 0 ? (int64_t)total + (DRAIN) : 0;                                  \
            FOLDIN_STATEMENTS LOAD                                                            \
          }                                                                                   \
        }                                                                                     \
      }                                                                                       \
      need = !finished && left == 0;                                                          \
    }                                                                                         \
  } while (0)

// A pipeline stage's place in its row is three locals: triples passed COUNT, epoch EPOCH and position POS of the
// next one.  Index of that triple among the launch's epochs * nnz, and the step on to the next.
#define FOLDIN_TRIPLE(EPOCH, POS) ((int64_t)(EPOCH) * nnz + (lo - base0) + (POS))
#define FOLDIN_ADVANCE(COUNT, EPOCH, POS, LEN) \
  do {                                         \
    ++COUNT;                                   \
    if (++POS == (LEN)) {                      \
      POS = 0;                                 \
      ++EPOCH;                                 \
    }                                          \
  } while (0)

namespace bpr {

// One fold-in step on the row a group holds in registers:
//   x = <p, q_i - q_j> + (b_i - b_j),  w = sigma(-x),  p <- p - lr (-w (q_i - q_j) + alpha_user p)   where `upd`.
// The dot is an fmaf chain over the lane's elements, then the group's DPP sum.  Both kernels call this and nothing
// else for the update, so a negative applied by either gives the same bits.  Wave-uniform call (group_sum).
template <int G, int E>
__device__ __forceinline__ void foldin_update(float (&p)[E], const float (&qi)[E], const float (&qj)[E], float bi,
                                              float bj, bool upd, float lr, float au, int lane) {
  float xl = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) xl = fmaf(p[e], qi[e] - qj[e], xl);
  float x = group_sum<G>(xl, lane);
  x += bi - bj;
  const float w = 1.0f / (1.0f + expf(x));
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float pe = p[e];
    const float du = -lr * (-w * (qi[e] - qj[e]) + au * pe);
    p[e] = upd ? pe + du : pe;
  }
}

// The step of the WARP objective (bpr_scored.h) on the row a group holds: foldin_update with the rank weight L in the
// place of sigma(-x) —  p <- p - lr (-L (q_i - q_j) + alpha_user p)  where `upd`.  L = 0 leaves the L2 term alone.  No
// reduction: the scores were the draw's business.
template <int G, int E>
__device__ __forceinline__ void foldin_update_warp(float (&p)[E], const float (&qi)[E], const float (&qj)[E], float L,
                                                   bool upd, float lr, float au) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float pe = p[e];
    const float du = -lr * (-L * (qi[e] - qj[e]) + au * pe);
    p[e] = upd ? pe + du : pe;
  }
}

// ---- host side (defined in bpr_foldin.hip).  `who`: the entry point's name, the head of every message.
int foldin_check_shape(const char* who, int64_t n, int64_t I, int32_t d);
// the `sampler` argument of an entry that draws uniformly or is given its negatives; `noun`: what it folds in
int foldin_check_sampler(const char* who, const char* noun, int32_t sampler);
// The one host read of a launch: the first and the last entry of `indptr` (rows + 1 entries, on the device), read
// on `stream` and waited for.  *nnz = their difference; refuses an indptr that does not ascend and
// epochs * nnz >= 2^31, the bound of the kernels' 32-bit triple counters.
int foldin_read_nnz(const char* who, const int64_t* indptr, int64_t rows, int32_t epochs, hipStream_t stream,
                    int64_t* nnz);
// A ticket word of the current device for one launch (the caller zeroes it in stream order) and the device's CU
// count.  Words are one 128-byte line each and handed out round-robin, so calls on different streams do not share
// one until 256 calls are in flight at once.
int foldin_next_ticket(const char* who, uint32_t** out, int* cus);
// foldin_next_ticket, and the word zeroed in stream order: what a launch does just before it plans its grid
int foldin_begin(const char* who, hipStream_t stream, uint32_t** ticket, int* cus);

}  // namespace bpr
