// bpr_plan.hip — the epoch planner (bpr_plan_epoch, bpr_plan_chunk): which triples make up which STREAM chunk.
#include <string.h>  // (rocprim's texture iterator calls the host memset)
#include <rocprim/device/device_radix_sort.hpp>

#include <stdlib.h>

#include <algorithm>

#include "bpr_ctx.h"

namespace bpr {

// ---------------------------------------------------------------------------------------------
// Epoch planner: DataLoader(shuffle=True) of the reference (example.py:307-321, exp.py:109-118)
// re-stated for the STREAM kernel.  A keyed Feistel network gives a pseudo-random permutation
// pi of [0, n) that every thread can evaluate on its own; triple t goes to chunk pi(t) / chunk,
// and one radix sort by (chunk, user) makes every chunk contiguous and grouped by user.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint64_t feistel_perm(uint64_t x, uint64_t n, int half_bits,
                                                 uint64_t seed) {
  const uint32_t mask = (half_bits >= 32) ? 0xFFFFFFFFu : ((1u << half_bits) - 1u);
  do {  // cycle-walk: the network permutes [0, 4^half_bits) ⊇ [0, n)
    uint32_t l = (uint32_t)(x >> half_bits) & mask, r = (uint32_t)x & mask;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
      const uint32_t k = (uint32_t)(seed >> (16 * (round & 1))) + 0x9E3779B9u * (uint32_t)(round + 1) +
                         (uint32_t)(seed >> 32);
      const uint32_t f = mix32(r ^ k) & mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = ((uint64_t)l << half_bits) | r;
  } while (x >= n);
  return x;
}

// K: uint32_t when (chunk, user) fits 32 bits — the usual case (ML-20M: 6 + 18 bits): the radix
// sort is bound by the bytes it moves, and 8-byte (key, value) pairs instead of 12 make it a third
// faster (0.49 -> 0.3 ms per 9.55 M-triple epoch) — else uint64_t
template <typename K>
__global__ void k_plan_keys(const int32_t* __restrict__ users, int64_t n, int64_t chunk,
                            int half_bits, int ubits, uint64_t seed, K* __restrict__ keys) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t c = feistel_perm((uint64_t)t, (uint64_t)n, half_bits, seed) / (uint64_t)chunk;
    keys[t] = (K)((c << ubits) | (uint64_t)(uint32_t)users[t]);
  }
}

template <typename K>
__global__ void k_plan_users(const K* __restrict__ keys, int64_t n, int ubits,
                             int32_t* __restrict__ users_out) {
  const uint64_t mask = (1ull << ubits) - 1ull;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    users_out[t] = (int32_t)((uint64_t)keys[t] & mask);
}

// the inverse permutation (same network run backwards, same cycle-walk): pi^-1(pi(t)) = t
__device__ __forceinline__ uint64_t feistel_inv(uint64_t y, uint64_t n, int half_bits, uint64_t seed) {
  const uint32_t mask = (half_bits >= 32) ? 0xFFFFFFFFu : ((1u << half_bits) - 1u);
  do {
    uint32_t l = (uint32_t)(y >> half_bits) & mask, r = (uint32_t)y & mask;
#pragma unroll
    for (int round = 3; round >= 0; --round) {
      const uint32_t k = (uint32_t)(seed >> (16 * (round & 1))) + 0x9E3779B9u * (uint32_t)(round + 1) +
                         (uint32_t)(seed >> 32);
      const uint32_t pr = l;                      // the forward round's input r
      const uint32_t pl = r ^ (mix32(pr ^ k) & mask);
      l = pl;
      r = pr;
    }
    y = ((uint64_t)l << half_bits) | r;
  } while (y >= n);
  return y;
}

// bpr_plan_chunk: the members of ONE chunk of the epoch plan, found through the inverse permutation
// (chunk c = pi^-1 of [c * chunk, (c + 1) * chunk)) instead of by sorting the whole epoch
__global__ void k_plan_chunk(const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                             int64_t n, int64_t j0, int64_t m, int half_bits, uint64_t seed,
                             uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t t = feistel_inv((uint64_t)(j0 + k), (uint64_t)n, half_bits, seed);
    keys[k] = (uint32_t)users[t];
    vals[k] = pos[t];
  }
}

// ---- grouping one chunk by user in three small kernels (the chunk is planned on the CU-masked side
// stream, where every kernel launch costs ~12 us: a device-wide radix sort of 199 k keys is NINE of
// them).  Users fall into nb <= 2048 buckets of 2^shift consecutive ids: (1) members + bucket
// histogram, (2) scatter into the buckets' ranges, (3) one workgroup per bucket orders its members by
// user with a counting sort over the bucket's 2^shift ids in LDS.  Output: users ascending, the
// order of one user's triples as the atomics fell.
constexpr int PC_MAX_BUCKETS = 2048, PC_MAX_LOCAL = 1024;

__global__ __launch_bounds__(256) void k_pc_members(const int32_t* __restrict__ users,
                                                    const int32_t* __restrict__ pos, int64_t n, int64_t j0,
                                                    int m, int half_bits, uint64_t seed, int shift,
                                                    uint32_t* __restrict__ mu, int32_t* __restrict__ mp,
                                                    uint32_t* __restrict__ cnt) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) {
    const uint64_t t = feistel_inv((uint64_t)(j0 + k), (uint64_t)n, half_bits, seed);
    const uint32_t u = (uint32_t)users[t];
    mu[k] = u;
    mp[k] = pos[t];
    atomicAdd(&cnt[u >> shift], 1u);
  }
}

__global__ __launch_bounds__(256) void k_pc_scatter(const uint32_t* __restrict__ mu,
                                                    const int32_t* __restrict__ mp, int m, int shift, int nb,
                                                    const uint32_t* __restrict__ cnt, uint32_t* __restrict__ cur,
                                                    uint32_t* __restrict__ base_out, uint32_t* __restrict__ bu,
                                                    int32_t* __restrict__ bp) {
  __shared__ uint32_t base[PC_MAX_BUCKETS];
  __shared__ uint32_t part[256];
  // exclusive scan of the bucket counts, redundantly in every workgroup (nb <= 2048: 8 per thread)
  const int per = (nb + 255) / 256;
  uint32_t acc = 0;
  for (int q = 0; q < per; ++q) {
    const int b = threadIdx.x * per + q;
    acc += b < nb ? cnt[b] : 0u;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int k = 0; k < 256; ++k) {
      const uint32_t v = part[k];
      part[k] = run;
      run += v;
    }
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (int q = 0; q < per; ++q) {
    const int b = threadIdx.x * per + q;
    if (b < nb) {
      base[b] = run;
      if (blockIdx.x == 0) base_out[b] = run;
      run += cnt[b];
    }
  }
  __syncthreads();
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) {
    const uint32_t u = mu[k];
    const uint32_t b = u >> shift;
    const uint32_t slot = base[b] + atomicAdd(&cur[b], 1u);
    bu[slot] = u;
    bp[slot] = mp[k];
  }
}

__global__ __launch_bounds__(128) void k_pc_group(const uint32_t* __restrict__ bu, const int32_t* __restrict__ bp,
                                                  int shift, uint32_t* __restrict__ cnt, uint32_t* __restrict__ cur,
                                                  const uint32_t* __restrict__ base, int32_t* __restrict__ users_out,
                                                  int32_t* __restrict__ pos_out) {
  __shared__ uint32_t c[PC_MAX_LOCAL], o[PC_MAX_LOCAL];
  const int b = blockIdx.x;
  const uint32_t lo = base[b], sz = cnt[b];
  const int L = 1 << shift;
  const uint32_t mask = (uint32_t)L - 1u;
  for (int k = threadIdx.x; k < L; k += blockDim.x) c[k] = 0u;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < sz; k += blockDim.x) atomicAdd(&c[bu[lo + k] & mask], 1u);
  __syncthreads();
  // exclusive scan over the bucket's ids (<= 1024): a segment per thread, the 128 segment sums by one
  __shared__ uint32_t seg[128];
  const int per = (L + 127) / 128;
  {
    uint32_t acc = 0;
    for (int q = 0; q < per; ++q) {
      const int k = threadIdx.x * per + q;
      acc += k < L ? c[k] : 0u;
    }
    seg[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int k = 0; k < 128; ++k) {
      const uint32_t v = seg[k];
      seg[k] = run;
      run += v;
    }
  }
  __syncthreads();
  {
    uint32_t run = seg[threadIdx.x];
    for (int q = 0; q < per; ++q) {
      const int k = threadIdx.x * per + q;
      if (k < L) {
        o[k] = run;
        run += c[k];
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < sz; k += blockDim.x) {
    const uint32_t u = bu[lo + k];
    const uint32_t slot = lo + atomicAdd(&o[u & mask], 1u);
    users_out[slot] = (int32_t)u;
    pos_out[slot] = bp[lo + k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // the counters of this bucket are zero again for the next chunk
    cnt[b] = 0u;
    cur[b] = 0u;
  }
}

static int bits_for(uint64_t v) {  // bits needed to represent values 0..v
  int b = 1;
  while ((v >> b) != 0) ++b;
  return b;
}

int plan_epoch_impl(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n,
                    int64_t chunk, uint64_t seed, int32_t* users_out, int32_t* pos_out) {
  if (n == 0) return BPR_OK;
  if (n >= ((int64_t)1 << 31)) {
    set_error("bpr_plan_epoch: n must be < 2^31");
    return BPR_ERR_UNSUPPORTED;
  }
  if (c->hot_key_ptr != pos_in || c->hot_key_n != n) {  // new training set: measure popularity
    if (int rc = hot_build_impl(c, pos_in, n)) return rc;
  }
  const int ubits = bits_for((uint64_t)(c->U - 1));
  const int64_t n_chunks = (n + chunk - 1) / chunk;
  const int cbits = bits_for((uint64_t)(n_chunks - 1));
  int half_bits = (bits_for((uint64_t)(n - 1)) + 1) / 2;
  if (half_bits < 1) half_bits = 1;
  if (c->plan_cap < n) {
    hipFree(c->plan_keys); hipFree(c->plan_keys_sorted); hipFree(c->plan_tmp);
    c->plan_keys = c->plan_keys_sorted = nullptr;
    c->plan_tmp = nullptr;
    c->plan_cap = 0;
    BPR_HIP_CHECK(hipMalloc(&c->plan_keys, sizeof(uint64_t) * n));
    BPR_HIP_CHECK(hipMalloc(&c->plan_keys_sorted, sizeof(uint64_t) * n));
    size_t bytes = 0;
    BPR_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, c->plan_keys,
                                                     c->plan_keys_sorted, pos_in, pos_out, (int)n,
                                                     0, 64, c->stream));
    size_t bytes32 = 0;
    BPR_HIP_CHECK(rocprim::radix_sort_pairs(
        nullptr, bytes32, reinterpret_cast<uint32_t*>(c->plan_keys),
        reinterpret_cast<uint32_t*>(c->plan_keys_sorted), pos_in, pos_out, (int)n, 0, 32, c->stream));
    bytes = std::max(bytes, bytes32);
    BPR_HIP_CHECK(hipMalloc(&c->plan_tmp, bytes > 0 ? bytes : 16));
    c->plan_tmp_bytes = bytes;
    c->plan_cap = n;
  }
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  size_t bytes = c->plan_tmp_bytes;  // sized for 64-bit keys: enough for 32-bit ones
  // (a sort on the bits [ubits, 32) of 32-bit keys goes to the 64-bit route: for a few thousand to a million keys
  // rocprim sorts by merging under the mask ((K)1 << end_bit) - 1 ^ ((K)1 << begin_bit) - 1, and a shift by the whole
  // width of K leaves the USER bits in that mask — the plan came out sorted by user, not by chunk.  begin_bit = 0
  // compares whole keys, no mask.)
  const bool keys32 = ubits + cbits <= 32 && !(c->tune_plan_sorted && ubits + cbits == 32);
  if (keys32) {
    uint32_t* k32 =reinterpret_cast<uint32_t*>(c->plan_keys);
    uint32_t* k32s = reinterpret_cast<uint32_t*>(c->plan_keys_sorted);
    hipLaunchKernelGGL(k_plan_keys<uint32_t>, dim3(grid), dim3(256), 0, c->stream, users_in, n,
                       chunk, half_bits, ubits, seed, k32);
    // (input promised sorted by user — bpr_set_tuning "plan_input_sorted": a STABLE sort on the chunk bits alone
    // leaves every chunk grouped by user, the same output in one radix pass instead of three)
    BPR_HIP_CHECK(rocprim::radix_sort_pairs(c->plan_tmp, bytes, k32, k32s, pos_in, pos_out,
                                                     (int)n, c->tune_plan_sorted ? ubits : 0, ubits + cbits, c->stream));
    hipLaunchKernelGGL(k_plan_users<uint32_t>, dim3(grid), dim3(256), 0, c->stream, k32s, n, ubits,
                       users_out);
  } else {
    hipLaunchKernelGGL(k_plan_keys<uint64_t>, dim3(grid), dim3(256), 0, c->stream, users_in, n,
                       chunk, half_bits, ubits, seed, c->plan_keys);
    BPR_HIP_CHECK(rocprim::radix_sort_pairs(c->plan_tmp, bytes, c->plan_keys,
                                                     c->plan_keys_sorted, pos_in, pos_out, (int)n,
                                                     c->tune_plan_sorted ? ubits : 0, ubits + cbits, c->stream));
    hipLaunchKernelGGL(k_plan_users<uint64_t>, dim3(grid), dim3(256), 0, c->stream,
                       c->plan_keys_sorted, n, ubits, users_out);
  }
  BPR_HIP_CHECK(hipGetLastError());
  c->plan_users = users_out;
  c->plan_pos = pos_out;
  c->plan_n = n;
  c->plan_chunk = chunk;
  return BPR_OK;
}

// One chunk of the plan (the same member set as chunk `index` of bpr_plan_epoch with the same seed,
// grouped by user), on `st`.  The plan does not depend on the model, so it can be computed for the
// chunk after next on the split refresh's side stream, in the time the sort leaves idle.
int plan_chunk_impl(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n, int64_t chunk,
                    uint64_t seed, int64_t index, int32_t* users_out, int32_t* pos_out, hipStream_t st) {
  const int64_t j0 = index * chunk;
  if (j0 >= n) return BPR_OK;
  const int64_t m = std::min<int64_t>(chunk, n - j0);
  int half_bits = (bits_for((uint64_t)(n - 1)) + 1) / 2;
  if (half_bits < 1) half_bits = 1;
  const int ubits = bits_for((uint64_t)(c->U - 1));
  if (c->pc_cap < m) {
    hipFree(c->pc_keys); hipFree(c->pc_vals); hipFree(c->pc_tmp);
    hipFree(c->pc_keys2); hipFree(c->pc_vals2); hipFree(c->pc_cnt);
    c->pc_keys = c->pc_keys2 = nullptr; c->pc_vals = c->pc_vals2 = nullptr; c->pc_tmp = nullptr;
    c->pc_cnt = nullptr;
    c->pc_cap = 0;
    BPR_HIP_CHECK(hipMalloc(&c->pc_keys, sizeof(uint32_t) * m));
    BPR_HIP_CHECK(hipMalloc(&c->pc_vals, sizeof(int32_t) * m));
    BPR_HIP_CHECK(hipMalloc(&c->pc_keys2, sizeof(uint32_t) * m));
    BPR_HIP_CHECK(hipMalloc(&c->pc_vals2, sizeof(int32_t) * m));
    BPR_HIP_CHECK(hipMalloc(&c->pc_cnt, sizeof(uint32_t) * 3 * PC_MAX_BUCKETS));
    BPR_HIP_CHECK(hipMemsetAsync(c->pc_cnt, 0, sizeof(uint32_t) * 3 * PC_MAX_BUCKETS, st));
    size_t bytes = 0;
    BPR_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, c->pc_keys,
                                                     reinterpret_cast<uint32_t*>(users_out), c->pc_vals,
                                                     pos_out, (int)m, 0, 32, st));
    BPR_HIP_CHECK(hipMalloc(&c->pc_tmp, bytes > 0 ? bytes : 16));
    c->pc_tmp_bytes = bytes;
    c->pc_cap = m;
  }
  const unsigned grid = (unsigned)std::min<int64_t>((m + 255) / 256, 1024);
  // three kernels when the users fit 2048 buckets of <= 1024 ids (U <= 2 M: every BASELINE shape);
  // BPR_PLAN_CHUNK_SORT=1 forces the device-wide sort (tests)
  const int shift = std::max(0, ubits - 11);
  static const bool force_sort = getenv("BPR_PLAN_CHUNK_SORT") != nullptr;
  if ((1 << shift) <= PC_MAX_LOCAL && !force_sort) {
    const int nb = (int)(((c->U - 1) >> shift) + 1);
    uint32_t *cnt = c->pc_cnt, *cur = c->pc_cnt + PC_MAX_BUCKETS, *base = c->pc_cnt + 2 * PC_MAX_BUCKETS;
    hipLaunchKernelGGL(k_pc_members, dim3(grid), dim3(256), 0, st, users_in, pos_in, n, j0, (int)m, half_bits,
                       seed, shift, c->pc_keys, c->pc_vals, cnt);
    hipLaunchKernelGGL(k_pc_scatter, dim3(std::min(grid, 256u)), dim3(256), 0, st, c->pc_keys, c->pc_vals, (int)m,
                       shift, nb, cnt, cur, base, c->pc_keys2, c->pc_vals2);
    hipLaunchKernelGGL(k_pc_group, dim3(nb), dim3(128), 0, st, c->pc_keys2, c->pc_vals2, shift, cnt, cur, base,
                       users_out, pos_out);
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  }
  hipLaunchKernelGGL(k_plan_chunk, dim3(grid), dim3(256), 0, st, users_in, pos_in, n, j0, m, half_bits,
                     seed, c->pc_keys, c->pc_vals);
  size_t bytes = c->pc_tmp_bytes;
  BPR_HIP_CHECK(rocprim::radix_sort_pairs(c->pc_tmp, bytes, c->pc_keys,
                                                   reinterpret_cast<uint32_t*>(users_out), c->pc_vals,
                                                   pos_out, (int)m, 0, ubits, st));
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

}  // namespace bpr
