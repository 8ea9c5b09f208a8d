// bpr_foldin_shared.h — what the fold-in kernels have in common.  The two user fold-in kernels (k_foldin,
// bpr_foldin.hip; k_foldin_adaptive, bpr_foldin_adaptive.hip) share the update of a user row by one triple; they and
// the item fold-in kernel (k_foldin_items, bpr_foldin_items.hip, which has an update of its own) share the shape
// check of their entry points and the ticket words their launches hand rows out with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpr_device.h"

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

// host side (defined in bpr_foldin.hip)
int foldin_check_shape(const char* who, int64_t n, int64_t I, int32_t d);
// A ticket word of the current device for one launch (the caller zeroes it in stream order) and the device's CU
// count.  Words are one 128-byte line each and handed out round-robin, so calls on different streams do not share
// one until 256 calls are in flight at once.
int foldin_next_ticket(const char* who, uint32_t** out, int* cus);

}  // namespace bpr
