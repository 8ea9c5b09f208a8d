// bpr_foldin_seen.h — "has the row's user seen item c?" for the fold-in kernels that draw their negatives from the
// live row (k_foldin_adaptive, bpr_foldin_adaptive.hip; k_foldin_scored, bpr_foldin_scored.hip): the two predicates of
// one set — a per-group I-bit bitmap in LDS, or the row's CSR slice — and the build of the bitmap.  Which one a launch
// takes is its plan's business (bpr_foldin_adaptive_plan.h, bpr_foldin_scored_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpr_device.h"

namespace bpr {

// An id outside [0, I) counts as seen, which is what the adaptive walk does with item 0: never a candidate.  `on`
// false: the empty row of a dummy draw.
struct SeenRowBits {
  const uint32_t* bm;
  int32_t I;
  bool on;
  __device__ __forceinline__ bool operator()(int32_t c) const {
    if ((uint32_t)c >= (uint32_t)I) return true;
    return on && ((bm[c >> 5] >> (c & 31)) & 1u) != 0u;
  }
};
struct SeenRowCsr {
  SeenCsr row;  // lo == hi: the empty row of a dummy draw
  int32_t I;
  __device__ __forceinline__ bool operator()(int32_t c) const {
    if ((uint32_t)c >= (uint32_t)I) return true;
    return row(c);
  }
};

// orders the LDS operations of one wave for the compiler (the hardware executes them in program order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace bpr

// The group's bitmap BM of the row it has just taken (items [lo, lo + m) of ITEMS), built once for the row's
// epochs * m draws.  A macro for the reason FOLDIN_NEXT_ROWS is one (a function changes the kernel's schedule); it
// names the kernel's `lo`, `m` and `gl`, and runs under the group's own predicate.  A group's bitmap is touched by its
// own lanes only, and a CSR item outside [0, NUM_ITEMS) is not entered.
#define FOLDIN_BUILD_BITMAP(LANES, BM, WORDS, ITEMS, NUM_ITEMS)                                                   \
  do {                                                                                                            \
    uint4* bm4 = reinterpret_cast<uint4*>(BM);                                                                    \
    for (int k = gl; k < ((WORDS) >> 2); k += (LANES)) bm4[k] = make_uint4(0u, 0u, 0u, 0u);                       \
    wave_lds_sync();                                                                                              \
    for (int32_t k = gl; k < m; k += 8 * (LANES)) {                                                               \
      int32_t it[8];                                                                                              \
      _Pragma("unroll") for (int q = 0; q < 8; ++q) it[q] = k + q * (LANES) < m ? (ITEMS)[lo + k + q * (LANES)] : -1; \
      _Pragma("unroll") for (int q = 0; q < 8; ++q)                                                               \
        if ((uint32_t)it[q] < (uint32_t)(NUM_ITEMS)) atomicOr(&(BM)[it[q] >> 5], 1u << (it[q] & 31));             \
    }                                                                                                             \
    wave_lds_sync();                                                                                              \
  } while (0)
