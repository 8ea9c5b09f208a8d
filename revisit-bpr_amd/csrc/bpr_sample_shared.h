// bpr_sample_shared.h — the draw of the sampling kernel (k_sample, bpr_sample.hip): which random bits a (row, item)
// pair gets, the uniform, the logarithm, the Gumbel noise and the key.  Every function here is a fixed sequence of
// integer and fp32 operations, written with the __f*_rn intrinsics so that neither -ffp-contract nor
// -fhip-fp32-correctly-rounded-divide-sqrt has anything to decide (no division, no square root, no libm, no fast
// intrinsic): the header means the same under the Makefile's two flag sets.  Like the chain of bpr_topk_shared.h
// this is a contract, not a detail: bpr_sample_rows' items and keys are a pure function of (tables, user, draw_id,
// seed, temperature), and whoever changes a step or a coefficient here changes every draw ever logged.  The host
// statement is tests/sample_model.py (numpy, a correctly rounded fma); tests/test_gpu_sample.py holds the kernel to
// its bits, tests/test_sample_model_cpu.py holds it to float64 over every uniform there is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpr_device.h"

namespace bpr {

// bpr_device.h has 0 and 1 (PURPOSE_UNIFORM, PURPOSE_ADAPTIVE), bpr_foldin_items_roles.hip has 2 (PURPOSE_ROLE)
constexpr uint32_t PURPOSE_GUMBEL = 3u;

// The random bits of (row, item i) are word i & 3 of this block: a block serves 4 consecutive ids, and the key is
// the pair, not the launch geometry.  draw_id: the row's 64-bit id (the user id unless the caller gives another).
__device__ __forceinline__ u32x4 sample_block(uint64_t seed, uint64_t draw_id, uint32_t item_block) {
  return philox4x32_10(item_block, (uint32_t)draw_id, (uint32_t)(draw_id >> 32), PURPOSE_GUMBEL, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// u = ((bits >> 9) + 0.5f) * 2^-23, strictly inside (0, 1), 2^23 distinct values.  Every step is exact: n < 2^23,
// so 2 n + 1 < 2^24 fits fp32's significand.  (One bit more does not: (n + 0.5f) with n >= 2^23 needs 25 bits, and
// n = 2^24 - 1 would round to u = 1 and a noise of +inf.)
__device__ __forceinline__ float sample_uniform(uint32_t bits) {
  return __fmul_rn(__fadd_rn((float)(bits >> 9), 0.5f), 1.1920928955078125e-07f);
}

// log(x) for a positive, normal, finite x.  x = m * 2^e with m in [sqrt(1/2), sqrt(2)) by integer operations on the
// bits, f = m - 1 (exact), log(1 + f) = f - f^2 / 2 + f^3 p(f) with the degree-8 p of Cephes' logf, e * ln 2 added
// in two pieces (LN2_HI has 11 significant bits: e * LN2_HI is exact).  Measured over all 2^23 uniforms against
// float64: g = -log(-log(u)) is off by at most 5.34e-7.
__device__ __forceinline__ float sample_log(float x) {
  const uint32_t ix = __float_as_uint(x) - 0x3F3504F3u;
  const float e = (float)((int32_t)ix >> 23);
  const float f = __fadd_rn(__uint_as_float((ix & 0x007FFFFFu) + 0x3F3504F3u), -1.0f);
  float p = 7.0376836292e-2f;
  p = __fmaf_rn(p, f, -1.1514610310e-1f);
  p = __fmaf_rn(p, f, 1.1676998740e-1f);
  p = __fmaf_rn(p, f, -1.2420140846e-1f);
  p = __fmaf_rn(p, f, 1.4249322787e-1f);
  p = __fmaf_rn(p, f, -1.6668057665e-1f);
  p = __fmaf_rn(p, f, 2.0000714765e-1f);
  p = __fmaf_rn(p, f, -2.4999993993e-1f);
  p = __fmaf_rn(p, f, 3.3333331174e-1f);
  const float z = __fmul_rn(f, f);
  const float t = __fmul_rn(f, z);
  float y = __fmul_rn(t, p);
  y = __fmaf_rn(e, -2.12194440e-4f, y);
  y = __fmaf_rn(-0.5f, z, y);
  const float r = __fadd_rn(f, y);
  return __fmaf_rn(e, 0.693359375f, r);
}

// g = -log(-log(u)): u in [2^-24, 1 - 2^-24], so -log(u) is in [5.9e-8, 16.7], positive and normal
__device__ __forceinline__ float sample_gumbel(uint32_t bits) {
  return -sample_log(-sample_log(sample_uniform(bits)));
}

// key = fmaf(score, inv_temp, g).  A NaN score gives a NaN key, a +-inf score a +-inf key.
__device__ __forceinline__ float sample_key(float score, float inv_temp, uint32_t bits) {
  return __fmaf_rn(score, inv_temp, sample_gumbel(bits));
}

}  // namespace bpr
