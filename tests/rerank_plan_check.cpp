// A stand-alone host program over revisit-bpr_amd/csrc/bpr_rerank_plan.h: tests/test_rerank_cpu.py compiles it with
// the host compiler under -fsanitize=address,undefined and runs it.  It sweeps the plan over shapes — among them row
// counts past 2^31 and the lengths and row counts around the cuts between the layouts — so that an overflow in the
// plan's integer arithmetic is a sanitizer report, and restates the invariants the launch relies on.  Exit status 0:
// all held.
#include <stdio.h>

#include "bpr_rerank_plan.h"

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
  const int64_t ns[] = {0, 1, 3, 4, 5, 70, 1023, 1024, 8191, 8192, 1 << 20, (1 << 20) + 1, 4 * (int64_t)(1 << 20) + 1,
                        ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 3};
  const int ds[] = {1, 8, 31, 32, 33, 128, 256, 1000, 1024};
  const int ks[] = {0, 1, 10, 100, 128};
  long plans = 0;
  for (int64_t n : ns)
    for (int d : ds)
      for (int k : ks)
        for (int layout = 0; layout <= RERANK_LAYOUTS; ++layout)
          for (int64_t len = 0; len <= RERANK_WAVE_MID_LEN + 2;  // (in steps of 8 between the two cuts)
               len += len > 2 * RERANK_WAVE_MAX_LEN && len < RERANK_WAVE_MID_LEN - 8 ? 8 : 1) {
            const RerankPlan p = plan_rerank(n, d, k, len, layout);
            ++plans;
            CHECK(p.layout == RERANK_WAVE || p.layout == RERANK_WG);
            if (layout != RERANK_AUTO) CHECK(p.layout == layout);
            else
              CHECK((p.layout == RERANK_WAVE) ==
                    ((len >= 1 && len <= 128) || (len >= 1 && len <= 1024 && n >= 1024) || n >= 8192));
            CHECK(p.tile == (p.layout == RERANK_WAVE ? 64 : 256) && p.tile <= RERANK_TILE);
            CHECK(p.rows_per_group * p.tile == RERANK_THREADS);  // one chain per thread
            CHECK(p.cap == k + p.tile && p.cap <= 64 * ((TOPK_MAX + p.tile) / 64));
            CHECK(p.groups >= 0 && p.groups * p.rows_per_group >= n && (p.groups - 1) * p.rows_per_group < n + (n == 0));
            CHECK(p.grid >= 0 && p.grid <= RERANK_GRID_MAX && p.grid <= p.groups && (p.grid > 0) == (n > 0));
            CHECK(p.grid * RERANK_THREADS < ((int64_t)1 << 32));
            CHECK(p.team_lds % 16 == 0 && p.lds == p.team_lds * (size_t)p.rows_per_group);
            CHECK(p.lds <= 65536 && p.lds <= RERANK_LDS_LIMIT);
          }
  const RerankPlan big = plan_rerank(((int64_t)1 << 31) + 5, 128, 10, 1000, RERANK_WG);
  CHECK(big.groups == ((int64_t)1 << 31) + 5 && big.grid == RERANK_GRID_MAX);
  const RerankPlan bigw = plan_rerank(((int64_t)1 << 31) + 5, 128, 10, 50, 0);
  CHECK(bigw.groups == ((int64_t)1 << 29) + 2 && bigw.grid == RERANK_GRID_MAX);
  printf("%ld plans, %d failures; lds at k=128 d=1024: wave %zu, workgroup %zu of %zu\n", plans, failures,
         plan_rerank(1, 1024, 128, 0, RERANK_WAVE).lds, plan_rerank(1, 1024, 128, 0, RERANK_WG).lds, RERANK_LDS_LIMIT);
  return failures != 0;
}
