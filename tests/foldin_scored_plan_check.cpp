// A stand-alone host program over revisit-bpr_amd/csrc/bpr_foldin_scored_plan.h: tests/test_foldin_scored_cpu.py
// compiles it with the host compiler under -fsanitize=address,undefined and runs it.  It holds the group shape and the
// prefetch depth of every width, the seen structure's flip exactly where a workgroup's bitmaps stop fitting, the LDS
// and residency bounds, the grid against rows and CUs, and that the plan's words are the adaptive plan's (one set of
// predicates serves both kernels).  Exit status 0: all held.
#include <stdio.h>

#include "bpr_foldin_scored_plan.h"

using namespace bpr;

static int failures = 0;
#define CHECK(c)                                    \
  do {                                              \
    if (!(c)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #c); \
      ++failures;                                   \
    }                                               \
  } while (0)

int main() {
  static_assert(BPR_NEG_DYNAMIC == 3 && BPR_NEG_WARP == 4, "the ABI's numbers of the kinds");
  static_assert(foldin_scored_pf(1) == FOLDIN_SCORED_PF && foldin_scored_pf(4) == FOLDIN_SCORED_PF, "full depth to E = 4");
  static_assert(foldin_scored_pf(16) >= 1, "never no ring");
  long plans = 0;
  const int64_t ns[] = {0, 1, 3, 4, 7, 8, 9, 1000, 3071, 3072, 3073, 4096, 8192, 8193, 138493, ((int64_t)1 << 31) - 1};
  const int64_t Is[] = {1, 2, 50, 300, 20109, 65535, 65536, 65537, 131071, 131072, 131073, 1000000, ((int64_t)1 << 30) + 1};
  for (int kind : {BPR_NEG_DYNAMIC, BPR_NEG_WARP})
    for (int d : {1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024})
      for (int64_t I : Is)
        for (int mode : {FOLDIN_SEEN_AUTO, FOLDIN_SEEN_CSR, FOLDIN_SEEN_BITMAP})
          for (int cus : {1, 8, 256, 304})
            for (int64_t n : ns) {
              const FoldinScoredPlan p = plan_foldin_scored(n, I, d, kind, cus, mode);
              const FoldinAdaptivePlan a = plan_foldin_adaptive(n, I, d, cus, mode);
              ++plans;
              CHECK(p.G == group_shape(d).G && p.E == group_shape(d).E && p.G * p.E >= d);
              CHECK(p.block == FOLDIN_BLOCK && p.groups_per_block == FOLDIN_BLOCK / p.G);
              CHECK(p.pf == foldin_pf_at(FOLDIN_SCORED_PF, p.E) && p.pf >= 1 && p.pf <= FOLDIN_SCORED_PF);
              // the seen structure is the adaptive kernel's, word for word
              CHECK(p.bitmap == a.bitmap && p.bm_words == a.bm_words && p.lds_bytes == a.lds_bytes);
              const int64_t need = foldin_bitmap_words(I) * 4 * p.groups_per_block;
              CHECK((p.bitmap == 1) == (mode != FOLDIN_SEEN_CSR && need <= FOLDIN_ADAPTIVE_LDS_MAX));
              if (p.bitmap) {
                CHECK(p.bm_words % 4 == 0 && (int64_t)p.bm_words * 32 >= I && p.lds_bytes == need);
              } else {
                CHECK(p.bm_words == 0 && p.lds_bytes == 0);
              }
              CHECK(p.lds_bytes <= FOLDIN_ADAPTIVE_LDS_MAX);
              CHECK(p.resident >= 1 && p.resident <= FOLDIN_RESIDENT && p.resident <= a.resident);
              CHECK(p.resident >= FOLDIN_RESIDENT - 1 || p.bitmap);  // the registers cost one workgroup at the most
              CHECK((int64_t)p.resident * p.lds_bytes <= FOLDIN_ADAPTIVE_LDS_CU);
              CHECK(p.resident == (p.bitmap ? std::min<int64_t>(foldin_scored_resident(p.E, kind, true),
                                                                FOLDIN_ADAPTIVE_LDS_CU / p.lds_bytes)
                                            : foldin_scored_resident(p.E, kind, false)));
              const int64_t cap = (int64_t)cus * p.resident * p.groups_per_block;
              CHECK(p.groups == std::min<int64_t>(n, cap));
              CHECK(p.grid == (p.groups + p.groups_per_block - 1) / p.groups_per_block);
              CHECK(p.grid <= (int64_t)cus * p.resident);
              CHECK((p.grid - 1) * p.groups_per_block < std::max<int64_t>(p.groups, 1));  // no workgroup without a group
            }
  // the instantiations whose VGPRs do not leave 4 waves per SIMD, and only those
  for (int kind : {BPR_NEG_DYNAMIC, BPR_NEG_WARP})
    for (int E : {1, 2, 4, 8, 16})
      for (int bm = 0; bm < 2; ++bm) {
        const bool low = bm == 1 && (E == 16 || (E == 4 && kind == BPR_NEG_DYNAMIC));
        CHECK(foldin_scored_resident(E, kind, bm != 0) == (low ? 3 : 4));
      }
  // the flips the issue names: G = 32 holds 8 bitmaps, G = 64 holds 4, in 64 KiB
  CHECK(plan_foldin_scored(100, 65536, 128, BPR_NEG_WARP).bitmap == 1);
  CHECK(plan_foldin_scored(100, 65537, 128, BPR_NEG_WARP).bitmap == 0);
  CHECK(plan_foldin_scored(100, 131072, 129, BPR_NEG_DYNAMIC).bitmap == 1);
  CHECK(plan_foldin_scored(100, 131073, 129, BPR_NEG_DYNAMIC).bitmap == 0);
  printf("%ld plans, %d failures\n", plans, failures);
  return failures != 0;
}
