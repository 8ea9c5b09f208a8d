// A stand-alone host program over revisit-bpr_amd/csrc/bpr_diversify_plan.h: tests/test_diversify_cpu.py compiles it
// with the host compiler under -fsanitize=address,undefined and runs it.  It sweeps the plan over every pool length,
// every layout argument and row counts past 2^31, so that an overflow in the plan's integer arithmetic is a sanitizer
// report, and restates the invariants the launch and the kernel's carving of LDS rely on.  Exit status 0: all held.
#include <stdio.h>

#include "bpr_diversify_plan.h"

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
  const int64_t ns[] = {0, 1, 3, 70, 1023, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 4 * (int64_t)(1 << 20) + 1,
                        ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 3};
  long plans = 0;
  for (int64_t n : ns)
    for (int C = 1; C <= DIVERSIFY_CMAX; ++C)
      for (int layout = 0; layout <= DIVERSIFY_LAYOUTS; ++layout) {
        const DiversifyPlan p = plan_diversify(n, C, layout);
        ++plans;
        CHECK(p.layout == DIVERSIFY_WG);
        CHECK(p.cpad % DIVERSIFY_TILE == 0 && p.cpad >= C && p.cpad - C < DIVERSIFY_TILE && p.cpad <= DIVERSIFY_CMAX);
        const int T = p.cpad / DIVERSIFY_TILE;
        CHECK(p.tiles == T * (T + 1) / 2 && p.tiles <= 10);
        CHECK(p.tiles <= 3 * (DIVERSIFY_THREADS / 64));  // a wave owns at most three tiles
        CHECK(p.cpad * (DIVERSIFY_KC / 4) <= 4 * DIVERSIFY_THREADS);  // a thread stages at most four 16-byte pieces
        CHECK(p.cpad <= 2 * 64);  // the candidates sit in the first two waves
        CHECK(p.grid >= 0 && p.grid <= DIVERSIFY_GRID_MAX && p.grid <= n && (p.grid > 0) == (n > 0));
        CHECK(p.grid * DIVERSIFY_THREADS < ((int64_t)1 << 32));
        const size_t by_hand = 4 * (size_t)p.tiles * 32 * 33 + 4 * (size_t)p.cpad * 36 + 12 * (size_t)p.cpad + 128;
        CHECK(p.lds == by_hand && p.lds % 16 == 0);
        CHECK((4 * (size_t)p.tiles * 32 * 33) % 16 == 0 && (4 * (size_t)p.cpad * 36) % 16 == 0);
        CHECK(p.lds <= 65536 && p.lds <= DIVERSIFY_LDS_LIMIT);
        CHECK(p.lds * (p.cpad <= 32 ? 8 : p.cpad <= 64 ? 7 : p.cpad <= 96 ? 4 : 2) <= DIVERSIFY_LDS_LIMIT);
      }
  const DiversifyPlan big = plan_diversify(((int64_t)1 << 31) + 5, 128, 0);
  CHECK(big.grid == DIVERSIFY_GRID_MAX && big.lds == 62336);
  printf("%ld plans, %d failures; lds at C = 32 / 64 / 96 / 128: %zu / %zu / %zu / %zu of %zu\n", plans, failures,
         plan_diversify(1, 32, 0).lds, plan_diversify(1, 64, 0).lds, plan_diversify(1, 96, 0).lds,
         plan_diversify(1, 128, 0).lds, DIVERSIFY_LDS_LIMIT);
  return failures != 0;
}
