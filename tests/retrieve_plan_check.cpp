// A stand-alone host program over revisit-bpr_amd/csrc/bpr_retrieve_plan.h: tests/test_retrieve_cpu.py compiles it
// with the host compiler under -fsanitize=address,undefined and runs it.  It sweeps the plan over shapes — among
// them user counts past 2^31 / TOPK_TU tiles and past 2^31 rows, every k, the catalogue sizes around the tile — so
// that an overflow in the plan's integer arithmetic is a sanitizer report, and restates the invariants the launch
// relies on.  Exit status 0: all held.
#include <stdio.h>

#include "bpr_retrieve_plan.h"

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
  const int64_t ns[] = {0, 1, 63, 64, 65, 130, 16319, 16320, 16321, 16384, 32768, 32769, 138493,
                        ((int64_t)1 << 31) / TOPK_TU + 1, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) + 5,
                        (((int64_t)1 << 31) + 7) * TOPK_TU, ((int64_t)1 << 40) + 3};
  const int64_t Is[] = {1, 2, 127, 128, 129, 5000, 20109, 1000003, ((int64_t)1 << 31) - 1};
  const int slices[] = {0, 1, 2, 3, 7, 8, 9, 63, 64};
  const int cuss[] = {1, 2, 256, 304};
  long plans = 0;
  for (int k = 1; k <= RETRIEVE_MAX; ++k) {
    const int cap = retrieve_cap(k);
    CHECK(cap >= k + TOPK_TI && cap >= 2 * k && cap <= 2 * RETRIEVE_MAX && (cap & (cap - 1)) == 0);
    CHECK(retrieve_lds_bytes(k) <= RETRIEVE_LDS_CU);
    CHECK(retrieve_max_slices(k) >= 1 && (int64_t)retrieve_max_slices(k) * k <= RETRIEVE_SLICE_K);
    if (k != 1 && k != 100 && k != 128 && k != 129 && k != 256 && k != 257 && k != 1000 && k != 1023 && k != 1024)
      continue;
    for (int64_t n : ns)
      for (int64_t I : Is)
        for (int s : slices)
          for (int cus : cuss) {
            const RetrievePlan p = plan_retrieve(n, I, k, s, cus);
            ++plans;
            CHECK(p.user_tiles * TOPK_TU >= n && (p.user_tiles - 1) * TOPK_TU < n + (n == 0));
            CHECK(p.item_tiles * TOPK_TI >= I && (p.item_tiles - 1) * TOPK_TI < I);
            CHECK(p.slices >= 1 && p.slices <= TOPK_MAX_SLICES && p.slices <= p.item_tiles);
            CHECK((int64_t)p.slices * k <= RETRIEVE_SLICE_K);
            if (s > 0) CHECK(p.slices <= s);
            CHECK(p.cap == cap);
            CHECK(p.lds == retrieve_lds_bytes(k) && p.lds <= RETRIEVE_LDS_CU);
            CHECK(p.merge_lds <= 64 * 1024 + 1024 && (p.merge_lds == 0) == (p.slices == 1));
            CHECK(p.units == p.user_tiles * p.slices);
            CHECK(p.grid >= 0 && p.grid <= p.units && p.grid <= 2 * (int64_t)cus && (p.grid > 0) == (n > 0));
            CHECK(p.grid * 256 < ((int64_t)1 << 32));
            CHECK(p.buf_bytes == p.grid * TOPK_TU * cap * 8 && p.buf_bytes <= 2 * (int64_t)cus * TOPK_TU * 2048 * 8);
            CHECK(p.part_bytes == (p.slices > 1 ? n * p.slices * k * 8 : 0) && p.part_bytes >= 0);
            CHECK(p.ws_bytes == p.part_bytes + p.buf_bytes);
            // the slices cover the item tiles exactly once, none empty
            int64_t prev = 0;
            CHECK(retrieve_slice_tile(p, 0) == 0 && retrieve_slice_tile(p, p.slices) == p.item_tiles);
            for (int j = 1; j <= p.slices; ++j) {
              const int64_t b = retrieve_slice_tile(p, j);
              CHECK(b > prev);
              prev = b;
            }
            const int64_t w = retrieve_workspace_bytes(n, I, k, s, cus);
            CHECK(w >= p.ws_bytes);
            if (s > 0) CHECK(w == p.ws_bytes);
          }
  }
  // never shrinking in n, and constant past the persistent grid's reach (the library's choice of slices)
  for (int k : {1, 128, 129, 1024}) {
    int64_t last = 0;
    for (int64_t n : ns) {
      if (n > ((int64_t)1 << 31) + 5) continue;  // (the list is ascending up to here)
      const int64_t w = retrieve_workspace_bytes(n, 20109, k, 0);
      CHECK(w >= last);
      last = w;
    }
    const int64_t far = ((int64_t)1 << 31) - 1;
    CHECK(retrieve_workspace_bytes(138493, 20109, k, 0) == retrieve_workspace_bytes(far, 20109, k, 0));
  }
  printf("%ld plans, %d failures; lds at k=1024: %zu of %zu, cap %d\n", plans, failures, retrieve_lds_bytes(1024),
         RETRIEVE_LDS_CU, retrieve_cap(1024));
  return failures != 0;
}
