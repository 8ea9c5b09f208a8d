// bpr_eval.hip — the one evaluation kernel of libbprcore: ROC-AUC of a block of score rows (r6).
//
// The reference's RocAucMany / RocAucManySlow (revisit_bpr/metrics/auc.py:70-130 of the reference: every
// (positive, negative) pair of a row; the ML-20M / MSD configs list it among their 14 metrics) compares
// [B, I, I] scores or loops over users in Python; the PyTorch-ROCm restatement here sorts every row
// (revisit_bpr/metrics/auc.py: one [B, I] sort per block, ~3/4 of an evaluation's time).  The quantity needs
// far less: per row, for each of its T positives the number of negatives scored strictly below it.  One workgroup
// per row: the T positive scores are ranked in LDS (counting, T^2 / 256 per thread: T is tens), every score of the
// row finds the number of positives <= it by binary search in LDS and bumps one bin of a (T + 1)-bin histogram; a
// prefix sum of the bins gives "scores strictly below positive p", minus the positives among them.  One pass over
// the scores.
//
// THE CONTRACT (include/bprcore.h at bpr_auc_rows; held bit for bit by tests/test_gpu_auc.py against
// tests/auc_model.py).  For a row with scores s[0 .. I) and the SET Pos of its listed ids:
//   wins = #{(p, n) : p in Pos, n not in Pos, s[p] > s[n]}   with IEEE '>': false whenever either side is NaN,
//                                                            -0 == +0, subnormals by value, +-inf ordinary values
//   T = |Pos|;  result = float32(float64(wins) / (float64(T) * float64(I - T)))
//   NaN for T == 0, for T == I (0 / 0) and for T > 4096 ("not computed": the caller's sort-based path takes the row).
// Preconditions that the kernel cannot check without a fault path: ids in [0, I), and unique within a row (a
// repeated id would be counted as two positives; evaluation.evaluate_topk removes repeats before the call).
//
// Where NaN goes.  The positives are ranked by a TOTAL order: non-NaN scores by value (ties by list index), every
// NaN above +inf (among themselves by list index).  So the ranks are a permutation of 0 .. T - 1 whatever the
// scores hold — every s_sorted slot that a later phase reads is written in this launch —, the K non-NaN positives
// fill s_sorted[0 .. K) in ascending order and the NaN positives sit behind them, where the upper-bound search of a
// non-NaN score never goes right of them (NaN <= x is false) and where the final sum stops: a NaN positive wins
// nothing.  A NaN score of the row is not binned at all: it is below no positive, so it is nobody's win, but it
// stays in I - T: a NaN negative is a pair that is lost.
#include <hip/hip_runtime.h>
#include <math.h>

#include "bpr_host.h"

namespace bpr {

constexpr int AUC_T_MAX = 4096;  // positives per row held in LDS (more: the caller's sort-based path)

__global__ __launch_bounds__(256) void k_auc_rows(const float* __restrict__ scores, int64_t I,
                                                  const int64_t* __restrict__ pos_indptr,
                                                  const int32_t* __restrict__ pos_items, float* __restrict__ auc) {
  __shared__ float s_sorted[AUC_T_MAX];
  __shared__ uint32_t s_hist[AUC_T_MAX + 1];
  const int64_t row = blockIdx.x;
  const int64_t p0 = pos_indptr[row];
  const int T = (int)(pos_indptr[row + 1] - p0);
  const float* __restrict__ s = scores + row * I;
  if (T <= 0 || T > AUC_T_MAX || (int64_t)T >= I) {  // no positives or no negatives: 0 / 0 as the metric classes;
    if (threadIdx.x == 0) auc[row] = nanf("");        // too many: NaN marks "not computed"
    return;
  }
  // rank the positives' scores (ascending, NaN last, ties by index): sorted[rank] = score  (staged through the
  // bins' LDS).  The order is total, so every slot 0 .. T - 1 of s_sorted is written
  float* const s_pos = reinterpret_cast<float*>(s_hist);
  for (int p = threadIdx.x; p < T; p += blockDim.x) s_pos[p] = s[pos_items[p0 + p]];
  __syncthreads();
  for (int p = threadIdx.x; p < T; p += blockDim.x) {
    const float sp = s_pos[p];
    const bool p_nan = sp != sp;
    int rank = 0;
    for (int q = 0; q < T; ++q) {
      const float sq = s_pos[q];
      const bool q_nan = sq != sq;
      const bool before = p_nan ? !q_nan : sq < sp;           // (sq < sp is false for a NaN sq)
      const bool equal = p_nan ? q_nan : sq == sp;
      rank += (before || (equal && q < p)) ? 1 : 0;
    }
    s_sorted[rank] = sp;
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= T; b += blockDim.x) s_hist[b] = 0u;
  __syncthreads();
  // every score of the row: bin = #{positives <= it}; a thread counts runs of one bin privately
  uint32_t run_bin = 0xFFFFFFFFu, run_cnt = 0u;
  for (int64_t j = threadIdx.x; j < I; j += blockDim.x) {
    const float sj = s[j];
    if (sj != sj) continue;  // NaN: below no positive (see the header)
    int lo = 0, hi = T;  // upper bound: first index with sorted > sj
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_sorted[mid] <= sj) lo = mid + 1; else hi = mid;
    }
    if ((uint32_t)lo == run_bin) {
      ++run_cnt;
    } else {
      if (run_cnt) atomicAdd(&s_hist[run_bin], run_cnt);
      run_bin = (uint32_t)lo;
      run_cnt = 1u;
    }
  }
  if (run_cnt) atomicAdd(&s_hist[run_bin], run_cnt);
  __syncthreads();
  // below[p] = scores strictly below sorted[p] = sum of bins 0..p; the positives among them = first index of
  // sorted[p]'s value (ties are not "strictly below")
  if (threadIdx.x == 0) {
    double wins = 0.0;
    uint64_t below = 0;
    int first_equal = 0;
    for (int p = 0; p < T; ++p) {
      if (s_sorted[p] != s_sorted[p]) break;  // the NaN positives, behind the others: no wins
      below += s_hist[p];
      if (p > 0 && s_sorted[p] != s_sorted[p - 1]) first_equal = p;
      wins += (double)(below - (uint64_t)first_equal);
    }
    auc[row] = (float)(wins / ((double)T * (double)(I - T)));
  }
}

}  // namespace bpr

extern "C" int bpr_auc_rows(const float* scores, int64_t n, int64_t I, const int64_t* pos_indptr,
                            const int32_t* pos_items, float* auc_out, void* hip_stream) {
  using namespace bpr;
  if (n < 0 || I <= 0 || (n > 0 && (!scores || !pos_indptr || !pos_items || !auc_out)))
    return fail(BPR_ERR_INVALID, "bpr_auc_rows: bad argument");
  if (n == 0) return BPR_OK;
  hipLaunchKernelGGL(k_auc_rows, dim3((unsigned)n), dim3(256), 0, (hipStream_t)hip_stream, scores, I, pos_indptr,
                     pos_items, auc_out);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}
