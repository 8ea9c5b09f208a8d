// A stand-alone host program over revisit-bpr_amd/csrc/bpr_sample_plan.h: tests/test_sample_model_cpu.py compiles it
// with the host compiler under -fsanitize=address,undefined and runs it.  It holds the plan's LDS to the CU for every
// k, and sweeps the slice and workspace arithmetic over shapes — among them user counts past 2^31 rows — so that an
// overflow in the plan's integer arithmetic is a sanitizer report.  Exit status 0: all held.
#include <stdio.h>

#include "bpr_sample_plan.h"

using namespace bpr;

static int failures = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      printf("FAILED line %d: %s\n", __LINE__, #c);                 \
      ++failures;                                                   \
    }                                                               \
  } while (0)

int main() {
  const int64_t ns[] = {0, 1, 63, 64, 65, 70, 130, 16319, 16320, 16321, 16384, 138493, ((int64_t)1 << 31) - 1,
                        ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 3};
  const int64_t Is[] = {1, 2, 9, 127, 128, 129, 300, 5000, 20109, 1000003, ((int64_t)1 << 31) - 1};
  const int slices[] = {0, 1, 2, 3, 7, 8, 9, 63, 64};
  const int cuss[] = {1, 2, 256, 304};
  static_assert(SAMPLE_LDS_CU == 163840, "the LDS of a CU");
  static_assert(SAMPLE_SCRATCH_BYTES == 1024 + 2048, "seen masks and partials");
  long plans = 0;
  for (int k = 1; k <= TOPK_MAX; ++k) {
    // the candidate stays at 8 bytes: k_topk's budget, and log_z's scratch lives in the staging area
    CHECK(sample_lds_bytes(k) <= SAMPLE_LDS_CU);
    CHECK(sample_lds_bytes(k) == topk_lds_bytes(k));
    CHECK(sample_lds_bytes(k) >= SAMPLE_STAGE_Q_BYTES + (size_t)TOPK_TU * (k + TOPK_TI) * 8);
    if (k != 1 && k != 10 && k != 100 && k != 127 && k != 128) continue;
    for (int64_t n : ns)
      for (int64_t I : Is)
        for (int s : slices)
          for (int cus : cuss)
            for (int want = 0; want < 2; ++want) {
              const SamplePlan p = plan_sample(n, I, k, s, want != 0, cus);
              const TopkPlan t = plan_topk(n, I, k, s, cus);
              ++plans;
              CHECK(p.topk.user_tiles * TOPK_TU >= n && (p.topk.user_tiles - 1) * TOPK_TU < n + (n == 0));
              CHECK(p.topk.item_tiles * TOPK_TI >= I && (p.topk.item_tiles - 1) * TOPK_TI < I);
              CHECK(p.topk.slices == t.slices && p.topk.slices >= 1 && p.topk.slices <= TOPK_MAX_SLICES);
              CHECK(p.topk.slices <= p.topk.item_tiles);
              if (s > 0) CHECK(p.topk.slices <= s);
              CHECK(p.topk.cap == k + TOPK_TI && p.topk.lds == sample_lds_bytes(k));
              CHECK((p.topk.merge_lds == 0) == (p.topk.slices == 1) && p.topk.merge_lds <= 64 * 1024 + 1024);
              CHECK(p.topk.ws_bytes == (p.topk.slices > 1 ? n * p.topk.slices * k * 8 : 0));
              CHECK(p.topk.ws_bytes % 8 == 0);  // log_z's pairs start 8-byte aligned
              CHECK(p.lz_bytes == (want ? n * p.topk.slices * 8 : 0) && p.lz_bytes >= 0);
              CHECK(p.ws_bytes == p.topk.ws_bytes + p.lz_bytes && p.ws_bytes >= 0);
              // the slices cover the item tiles exactly once, none empty
              int64_t prev = 0;
              CHECK(topk_slice_tile(p.topk, 0) == 0 && topk_slice_tile(p.topk, p.topk.slices) == p.topk.item_tiles);
              for (int j = 1; j <= p.topk.slices; ++j) {
                const int64_t b = topk_slice_tile(p.topk, j);
                CHECK(b > prev);
                prev = b;
              }
              const int64_t w = sample_workspace_bytes(n, I, k, s, want != 0, cus);
              CHECK(w >= p.ws_bytes);
              if (s > 0) CHECK(w == p.ws_bytes);
              if (!want) CHECK(w == topk_workspace_bytes(n, I, k, s, cus));
            }
  }
  // never shrinking in n (the library's choice of slices)
  for (int k : {1, 128})
    for (int want = 0; want < 2; ++want) {
      int64_t last = 0;
      for (int64_t n : ns) {
        const int64_t w = sample_workspace_bytes(n, 20109, k, 0, want != 0);
        CHECK(w >= last);
        last = w;
      }
    }
  printf("%ld plans, %d failures; lds at k=128: %zu of %zu\n", plans, failures, sample_lds_bytes(128), SAMPLE_LDS_CU);
  return failures != 0;
}
