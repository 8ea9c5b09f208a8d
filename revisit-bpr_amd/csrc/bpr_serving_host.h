// bpr_serving_host.h — the host prologue the serving entry points share (bpr_topk.hip, bpr_retrieve.hip,
// bpr_sample.hip, bpr_neighbors.hip, bpr_rank.hip; the launch and vec_path also bpr_rerank.hip and
// bpr_diversify.hip), each piece once: the shape check, the small refusals, the split of the workspace into the
// slices' partial lists, the test for the vector path, the launch, the merge of the slices and the slice bounds
// of the test hooks.  Host code only: bpr_topk_shared.h is the device side.
//
// A helper takes no decision of its own.  Every entry point calls the pieces in ITS order, and where two entry
// points word or condition a refusal differently the difference is a parameter (DESIGN.md lists those
// differences): which refusal a malformed call meets, and in which words, is what it was before the pieces were
// shared (tests/test_serving_refusals_cpu.py holds every message).  `who` is the entry point's name, the head of
// every message.  The helpers have internal linkage, so the library's dynamic symbols stay the entry points'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "bpr_host.h"
#include "bpr_topk_plan.h"

namespace bpr {

// ---- the shape check, clause by clause in the order of check_topk_shape.  The rows of the table are `rows_name`
// in the messages ("I", "N").
static inline int check_table_shape(const char* who, int64_t n, int64_t rows, int32_t d, const char* rows_name) {
  if (n < 0 || rows < 1 || rows >= ((int64_t)1 << 31))
    return fail(BPR_ERR_INVALID, std::string(who) + ": n must be >= 0 and " + rows_name + " in [1, 2^31)");
  if (d < 1 || d > 1024) return fail(BPR_ERR_INVALID, std::string(who) + ": d must be in [1, 1024]");
  return BPR_OK;
}

static inline int check_item_slices(const char* who, int32_t item_slices, int max_slices) {
  if (item_slices < 0 || item_slices > max_slices)
    return fail(BPR_ERR_INVALID, std::string(who) + ": item_slices must be 0 (choose) or in [1, " +
                                     std::to_string(max_slices) + "]");
  return BPR_OK;
}

// the shape of a top-k call of k <= k_max over a table of `rows` rows (bpr_rank.hip has no k and its own bound on n:
// it calls the two pieces above and adds that bound)
static inline int check_topk_shape(const char* who, int64_t n, int64_t rows, int32_t d, int32_t k, int k_max,
                                   int32_t item_slices, const char* rows_name) {
  if (int rc = check_table_shape(who, n, rows, d, rows_name)) return rc;
  if (k < 1 || k > k_max)
    return fail(BPR_ERR_INVALID, std::string(who) + ": k must be in [1, " + std::to_string(k_max) + "]");
  if (int rc = check_item_slices(who, item_slices, TOPK_MAX_SLICES)) return rc;
  if (n > 0x7FFFFFFF)  // (the merge kernel's grid is one workgroup per row)
    return fail(BPR_ERR_INVALID, std::string(who) + ": n must be below 2^31");
  return BPR_OK;
}

// ---- the small refusals
// the out-pointer of a `_workspace` / `_slices` entry
static inline int check_out(const char* who, const void* out, const char* name) {
  if (out == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": " + name + " is NULL");
  return BPR_OK;
}

// The workspace of `<family>_rows`, which `<family>_workspace` sizes: NULL or too small for the `need` bytes.
// aligned_subject: nullptr, or the subject of "<subject> must be 8-byte aligned" (the two entry points that ask
// for it word it differently); align_unneeded: ask it of a workspace the shape does not need as well; rows: what
// follows the family in the entry point's name ("_rows_filtered").
static inline int check_workspace(const char* family, const void* workspace, int64_t have, int64_t need,
                                  const char* aligned_subject = nullptr, bool align_unneeded = false,
                                  const char* rows = "_rows") {
  const std::string who = std::string(family) + rows;
  if (need > 0 && (workspace == nullptr || have < need))
    return fail(BPR_ERR_INVALID, who + ": workspace of " + std::to_string(have) + " bytes, " + std::to_string(need) +
                                     " needed (" + family + "_workspace)");
  if (aligned_subject != nullptr && (need > 0 || align_unneeded) && reinterpret_cast<uintptr_t>(workspace) % 8 != 0)
    return fail(BPR_ERR_INVALID, who + ": " + aligned_subject + " must be 8-byte aligned");
  return BPR_OK;
}

// the item filter of a `_rows_filtered` entry (bpr_item_filter.h): NULL is no filter; a tile's four words are read as
// one 16-byte run
static inline int check_item_filter(const char* who, const void* item_filter) {
  if (reinterpret_cast<uintptr_t>(item_filter) % 16 != 0)
    return fail(BPR_ERR_INVALID, std::string(who) + ": item_filter must be 16-byte aligned");
  return BPR_OK;
}

// ---- where the scoring kernel of a sliced call writes: with several slices the partial lists at the head of the
// workspace ([n, S, k] scores, then as many ids), which launch_topk_merge reads; with one slice the caller's outputs
static inline void slice_outputs(void* workspace, int64_t n, int S, int k, float* out_s, int32_t* out_i,
                                 float** kernel_s, int32_t** kernel_i) {
  float* const part_s = reinterpret_cast<float*>(workspace);
  *kernel_s = S > 1 ? part_s : out_s;
  *kernel_i = S > 1 ? reinterpret_cast<int32_t*>(part_s + n * (int64_t)S * k) : out_i;
}

// ---- the vector path (16-byte global loads): d % 4 == 0 and 16-byte aligned tables
static inline bool vec_path(int d, const void* A, const void* B = nullptr) {
  return d % 4 == 0 && (reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) % 16 == 0;
}

// ---- the launch.  max_lds: the largest dynamic LDS the kernel may ever ask for; past 64 KiB that is a per-function
// attribute, set on every call (the process may hold several devices, and the call costs nothing next to a launch)
// and on the instantiation that is launched.  0: the kernel stays below 64 KiB and the attribute is left alone.
// Which instantiation runs is the caller's choice: it hands in the kernel.
template <typename... Params, typename... Args>
static inline int launch_kernel(void (*kernel)(Params...), size_t max_lds, dim3 grid, dim3 block, size_t lds,
                                hipStream_t stream, const Args&... args) {
  if (max_lds > 0)
    BPR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  BPR_HIP_CHECK(hipGetLastError());
  return BPR_OK;
}

// ---- the merge of the slices (k_topk_merge, bpr_topk.hip, where this is defined): per row the S sorted lists of k
// in part_s / part_i ([n, S, k], padded with id -1 at the end) -> the k best, sorted, in out_s / out_i ([n, k]).
// One slice: nothing to merge, nothing is launched.  merge_lds: TopkPlan::merge_lds.
int launch_topk_merge(const float* part_s, const int32_t* part_i, int64_t n, int S, int k, size_t merge_lds,
                      float* out_s, int32_t* out_i, hipStream_t stream);

// ---- the test hooks: bounds[0 .. slices] = the first table row of each slice, then `rows`
template <typename Plan>
static inline void slice_bounds(const Plan& p, int64_t (*slice_tile)(const Plan&, int), int tile_rows, int64_t rows,
                                int64_t* bounds) {
  for (int s = 0; s <= p.slices; ++s) bounds[s] = std::min<int64_t>(slice_tile(p, s) * tile_rows, rows);
}

}  // namespace bpr
