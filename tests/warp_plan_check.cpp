// A stand-alone host program over revisit-bpr_amd/csrc/bpr_scored_plan.h and bpr_stream_plan.h:
// tests/test_warp_model_cpu.py compiles it with the host compiler under -fsanitize=address,undefined and runs it.
// It holds the range of max_sampled and of the margin, the argument checks and the grid of the stand-alone kernel,
// the STREAM plan of a WARP launch — the uniform sampler's "seen?" structures, never the LDS tier — and that the
// plans of a uniform, an adaptive and a dynamic launch are what they were before the kind existed, over the sweep
// tests/dynamic_plan_check.cpp uses.  Exit status 0: all held.
#include <math.h>
#include <stdio.h>

#include <limits>

#include "bpr_scored_plan.h"
#include "bpr_stream_plan.h"

using namespace bpr;

static int failures = 0;
#define CHECK(c)                                    \
  do {                                              \
    if (!(c)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #c); \
      ++failures;                                   \
    }                                               \
  } while (0)

static StreamShape ml20m(int sampler) {
  StreamShape s = {};
  s.n = 265216; s.I = 20109; s.d = 128; s.G = 32; s.E = 4;
  s.sampler = sampler; s.cap_groups = 34169; s.run_len = 0; s.force_seen = SEEN_BY_SHAPE;
  s.cus = 256; s.grid_cap = STREAM_MAX_GRID;
  s.hot = true; s.hot_H = 256; s.tune_hot_lds = 256; s.tune_hot_lds_force = false;
  s.tune_lds_block = 0; s.tune_lds_tail = 10; s.lds_allowed = true;
  return s;
}

static bool same(const StreamPlan& a, const StreamPlan& b) {
  return a.kernel == b.kernel && a.seen == b.seen && a.block == b.block && a.grid == b.grid && a.shmem == b.shmem &&
         a.bm_words == b.bm_words && a.gpw_active == b.gpw_active && a.run_len == b.run_len && a.L == b.L &&
         a.tail1 == b.tail1 && a.tail2 == b.tail2;
}

static ScoredShape good() {
  ScoredShape s = {};
  s.kind = BPR_NEG_WARP;
  s.B = 8; s.I = 300; s.d = 32; s.count = 10; s.margin = 1.0f;
  s.have_users = s.have_pos = s.have_neg = s.have_tries = s.have_seen = true;
  return s;
}

int main() {
  static_assert(BPR_NEG_WARP == 4, "the ABI's number of the kind");
  static_assert(WARP_MIN == 1 && WARP_MAX == 32 && WARP_DEFAULT == 10, "the range of max_sampled and its default");
  CHECK(WARP_DEFAULT_MARGIN == 1.0f);
  CHECK(sampler_scored(BPR_NEG_DYNAMIC) && sampler_scored(BPR_NEG_WARP) && !sampler_scored(BPR_NEG_GIVEN) &&
        !sampler_scored(BPR_NEG_UNIFORM) && !sampler_scored(BPR_NEG_ADAPTIVE) && !sampler_scored(5) && !sampler_scored(-1));
  // ---- the ranges
  for (int64_t m : {(int64_t)-5, (int64_t)0, (int64_t)33, (int64_t)64, (int64_t)1 << 40}) CHECK(!warp_max_sampled_ok(m));
  for (int64_t m = 1; m <= 32; ++m) CHECK(warp_max_sampled_ok(m));
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float m : {0.f, -0.f, -1.f, inf, -inf, nan}) CHECK(!warp_margin_ok(m));
  for (float m : {1e-30f, 0.1f, 1.f, 100.f, 3e38f}) CHECK(warp_margin_ok(m));
  // ---- the stand-alone kernel: checks and grid
  long plans = 0;
  const int64_t Bs[] = {0, 1, 3, 4, 5, 7, 8, 9, 2048, 16383, 16384, 16385, ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 3};
  for (int64_t B : Bs)
    for (int d : {1, 20, 32, 64, 128, 129, 256, 512, 1024})
      for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)10, (int64_t)32, (int64_t)33})
        for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)1 << 20}) {
          ScoredShape s = good();
          s.B = B; s.d = d; s.count = m; s.grid_cap = cap;
          const ScoredPlan p = plan_scored(s);
          ++plans;
          if (m < 1 || m > 32) {
            CHECK(p.rc == BPR_ERR_INVALID && p.grid == 0);
            continue;
          }
          CHECK(p.rc == BPR_OK && p.block == 256 && p.G == group_shape(d).G && p.E == group_shape(d).E);
          const int64_t per_block = 256 / p.G, limit = cap > 0 && cap < WARP_MAX_GRID ? cap : WARP_MAX_GRID;
          CHECK((p.grid == 0) == (B == 0));
          CHECK((int64_t)p.grid <= limit);
          // every draw has a group, or the grid is at its cap (the kernel strides)
          CHECK((int64_t)p.grid * per_block >= B || (int64_t)p.grid == limit);
          if (B > 0) CHECK(((int64_t)p.grid - 1) * per_block < B);
          CHECK(p.chunks == (int)((m + dynamic_inflight_rows(p.E) - 1) / dynamic_inflight_rows(p.E)));
        }
  {
    const ScoredShape s = good();
    CHECK(plan_scored(s).rc == BPR_OK);
    ScoredShape t = s; t.have_users = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_pos = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_neg = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_tries = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_seen = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.B = -1;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.d = 0;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.d = 1025;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    for (float m : {0.f, -1.f, inf, nan}) {
      t = s; t.margin = m;
      CHECK(plan_scored(t).rc == BPR_ERR_INVALID && plan_scored(t).grid == 0);
    }
  }
  // ---- STREAM: the LDS tier is taken for uniform and adaptive at the timed shape, never for dynamic or WARP; the
  // "seen?" structure of a WARP launch is the uniform launch's
  {
    const int occ = 8;
    const StreamShape su = ml20m(BPR_NEG_UNIFORM), sa = ml20m(BPR_NEG_ADAPTIVE), sd = ml20m(BPR_NEG_DYNAMIC),
                      sw = ml20m(BPR_NEG_WARP);
    const StreamPlan pu = plan_stream(su, plan_stream_block(su), occ), pa = plan_stream(sa, plan_stream_block(sa), occ),
                     pd = plan_stream(sd, plan_stream_block(sd), occ), pw = plan_stream(sw, plan_stream_block(sw), occ);
    // the plans of the existing samplers, field by field, as the parent commit computes them
    const StreamPlan want_lds = {STREAM_LDS, STREAM_SEEN_BITMAP, 1024, 256, 162424, 632, 2, 8, 158, 238688, 254600};
    const StreamPlan want_plain = {STREAM_PLAIN, STREAM_SEEN_BITMAP, 256, 2763, 20224, 632, 2, 8, 0, 0, 0};
    CHECK(same(pu, want_lds));
    CHECK(same(pa, want_lds));
    CHECK(same(pd, want_plain));
    CHECK(same(pw, want_plain));
    // every way the tier can be asked for: WARP never takes it and plans as the uniform launch without the tier;
    // uniform, adaptive and dynamic plan as they did (dynamic as uniform without the tier, the others with it)
    for (int force = 0; force <= 3; ++force)
      for (int always = 0; always < 2; ++always)
        for (int64_t n : {(int64_t)1000, (int64_t)265216, (int64_t)4000000}) {
          StreamShape s = sw;
          s.force_seen = force; s.tune_hot_lds_force = always != 0; s.n = n;
          StreamPlan p = plan_stream_block(s);
          CHECK(!plan_stream_lds(s, p));
          const StreamPlan w = plan_stream(s, plan_stream_block(s), occ);
          CHECK(w.kernel == STREAM_PLAIN && w.L == 0);
          StreamShape u = s;
          u.sampler = BPR_NEG_UNIFORM; u.tune_hot_lds = 0;
          const StreamPlan plain_u = plan_stream(u, plan_stream_block(u), occ);
          CHECK(same(w, plain_u));
          StreamShape dy = s;
          dy.sampler = BPR_NEG_DYNAMIC;
          CHECK(same(plan_stream(dy, plan_stream_block(dy), occ), plain_u));
          // with the tier asked for, uniform and adaptive take it exactly when the parent's rule says so
          for (int smp : {BPR_NEG_UNIFORM, BPR_NEG_ADAPTIVE}) {
            StreamShape t = s;
            t.sampler = smp;
            const StreamPlan pt = plan_stream(t, plan_stream_block(t), occ);
            const bool fills = (n + 7) / 8 >= 2 * (int64_t)t.cus * (1024 / 64) * 2;
            CHECK((pt.kernel == STREAM_LDS) == (force != FORCE_CSR && (fills || always != 0)));
            CHECK(pt.seen == (force == FORCE_CSR ? STREAM_SEEN_CSR : force == FORCE_LIST ? STREAM_SEEN_LIST : STREAM_SEEN_BITMAP));
          }
        }
    // a large catalogue: the staged lists, as uniform
    StreamShape big = sw;
    big.I = 200000;
    CHECK(plan_stream_block(big).seen == STREAM_SEEN_LIST);
    StreamShape bigu = big;
    bigu.sampler = BPR_NEG_UNIFORM; bigu.tune_hot_lds = 0;
    CHECK(same(plan_stream(big, plan_stream_block(big), occ), plan_stream(bigu, plan_stream_block(bigu), occ)));
  }
  printf("%ld plans, %d failures\n", plans, failures);
  return failures != 0;
}
