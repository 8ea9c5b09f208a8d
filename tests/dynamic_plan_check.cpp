// A stand-alone host program over revisit-bpr_amd/csrc/bpr_scored_plan.h, bpr_group_shape.h and bpr_stream_plan.h:
// tests/test_dynamic_model_cpu.py compiles it with the host compiler under -fsanitize=address,undefined and runs it.
// It holds the range of M, the argument checks and the grid of the stand-alone kernel, the group shape every width
// gets — the fold-in plan's (bpr_foldin_plan.h) included —, the STREAM plan's refusal of the LDS tier for dynamic
// negatives — and that the plans of a uniform and an adaptive launch are what they were before the sampler existed.
// Exit status 0: all held.
#include <stdio.h>

#include "bpr_foldin_plan.h"
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

int main() {
  static_assert(BPR_NEG_DYNAMIC == 3, "the ABI's number of the sampler");
  static_assert(DYNAMIC_MIN == 1 && DYNAMIC_MAX == 32 && DYNAMIC_DEFAULT == 4, "the range of M and its default");
  // ---- the range of M
  for (int64_t m : {(int64_t)-5, (int64_t)0, (int64_t)33, (int64_t)64, (int64_t)1 << 40}) CHECK(!dynamic_candidates_ok(m));
  for (int64_t m = 1; m <= 32; ++m) CHECK(dynamic_candidates_ok(m));
  // ---- the group shape of every width: what bpr_bind_tables has always chosen
  for (int d = 1; d <= 1024; ++d) {
    const GroupShape g = group_shape(d);
    CHECK(g.G == (d <= 128 ? 32 : 64));
    CHECK(g.G * g.E >= d);
    CHECK(g.E == 1 || g.E == 2 || g.E == 4 || g.E == 8 || g.E == 16);
    CHECK(g.E == (g.G == 32 ? 1 : 4) || g.G * g.E / 2 < d);  // the smallest E that holds the row
    CHECK(dynamic_inflight_rows(g.E) * g.E <= 32 && dynamic_inflight_rows(g.E) >= 2);
    // the fold-in plan's group shape is this one (it used to restate the rule: the value it had is the one held above)
    const FoldinPlan f = plan_foldin(1000, d);
    CHECK(f.G == g.G && f.E == g.E && f.G == (d <= 128 ? 32 : 64) && f.groups_per_block == FOLDIN_BLOCK / g.G);
    int fG = 0, fE = 0;
    foldin_ge(d, &fG, &fE);
    CHECK(fG == g.G && fE == g.E);
  }
  CHECK(group_shape(128).E == 4 && group_shape(129).G == 64 && group_shape(256).E == 4 && group_shape(257).E == 8 &&
        group_shape(20).E == 1 && group_shape(33).E == 2 && group_shape(1024).E == 16);
  // ---- the stand-alone kernel: checks and grid
  long plans = 0;
  const int64_t Bs[] = {0, 1, 3, 4, 5, 7, 8, 9, 2048, 16383, 16384, 16385, ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 3};
  for (int64_t B : Bs)
    for (int d : {1, 20, 32, 64, 128, 129, 256, 512, 1024})
      for (int64_t m : {(int64_t)0, (int64_t)1, (int64_t)4, (int64_t)32, (int64_t)33})
        for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)1 << 20}) {
          ScoredShape s = {};
          s.kind = BPR_NEG_DYNAMIC;
          s.B = B; s.I = 300; s.d = d; s.count = m; s.have_users = s.have_neg = s.have_seen = true; s.grid_cap = cap;
          const ScoredPlan p = plan_scored(s);
          ++plans;
          if (m < 1 || m > 32) {
            CHECK(p.rc == BPR_ERR_INVALID && p.grid == 0);
            continue;
          }
          CHECK(p.rc == BPR_OK && p.block == 256 && p.G == group_shape(d).G && p.E == group_shape(d).E);
          const int64_t per_block = 256 / p.G, limit = cap > 0 && cap < DYNAMIC_MAX_GRID ? cap : DYNAMIC_MAX_GRID;
          CHECK((p.grid == 0) == (B == 0));
          CHECK((int64_t)p.grid <= limit);
          // every draw has a group, or the grid is at its cap (the kernel strides)
          CHECK((int64_t)p.grid * per_block >= B || (int64_t)p.grid == limit);
          if (B > 0) CHECK(((int64_t)p.grid - 1) * per_block < B);
          CHECK(p.chunks == (int)((m + dynamic_inflight_rows(p.E) - 1) / dynamic_inflight_rows(p.E)));
        }
  {
    ScoredShape s = {};
    s.kind = BPR_NEG_DYNAMIC;
    s.B = 8; s.I = 300; s.d = 32; s.count = 4; s.have_users = s.have_neg = s.have_seen = true;
    CHECK(plan_scored(s).rc == BPR_OK);
    ScoredShape t = s; t.have_users = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_neg = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.have_seen = false;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.B = -1;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.d = 0;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
    t = s; t.d = 1025;
    CHECK(plan_scored(t).rc == BPR_ERR_INVALID);
  }
  // ---- STREAM: the LDS tier is taken for uniform and adaptive at the timed shape, never for dynamic; the "seen?"
  // structure of a dynamic launch is the uniform launch's
  {
    const int occ = 8;
    const StreamShape su = ml20m(BPR_NEG_UNIFORM), sa = ml20m(BPR_NEG_ADAPTIVE), sd = ml20m(BPR_NEG_DYNAMIC);
    const StreamPlan pu = plan_stream(su, plan_stream_block(su), occ), pa = plan_stream(sa, plan_stream_block(sa), occ),
                     pd = plan_stream(sd, plan_stream_block(sd), occ);
    // the plans of the two existing samplers, field by field, as the parent commit computes them
    const StreamPlan want_lds = {STREAM_LDS, STREAM_SEEN_BITMAP, 1024, 256, 162424, 632, 2, 8, 158, 238688, 254600};
    CHECK(same(pu, want_lds));
    CHECK(same(pa, want_lds));
    CHECK(pd.kernel == STREAM_PLAIN && pd.L == 0 && pd.block == 256);
    StreamShape plain_u = su;
    plain_u.tune_hot_lds = 0;  // the uniform launch without the tier: the plain plan the dynamic launch must share
    const StreamPlan ppu = plan_stream(plain_u, plan_stream_block(plain_u), occ);
    const StreamPlan want_plain = {STREAM_PLAIN, STREAM_SEEN_BITMAP, 256, 2763, 20224, 632, 2, 8, 0, 0, 0};
    CHECK(same(ppu, want_plain));
    CHECK(same(pd, ppu));
    // every way the tier can be asked for
    for (int force = 0; force <= 3; ++force)
      for (int always = 0; always < 2; ++always)
        for (int64_t n : {(int64_t)1000, (int64_t)265216, (int64_t)4000000}) {
          StreamShape s = sd;
          s.force_seen = force; s.tune_hot_lds_force = always != 0; s.n = n;
          StreamPlan p = plan_stream_block(s);
          CHECK(!plan_stream_lds(s, p));
          CHECK(plan_stream(s, plan_stream_block(s), occ).kernel == STREAM_PLAIN);
          StreamShape u = s;
          u.sampler = BPR_NEG_UNIFORM; u.tune_hot_lds = 0;
          CHECK(same(plan_stream(s, plan_stream_block(s), occ), plan_stream(u, plan_stream_block(u), occ)));
        }
    // a large catalogue: the staged lists, as uniform
    StreamShape big = sd;
    big.I = 200000;
    CHECK(plan_stream_block(big).seen == STREAM_SEEN_LIST);
  }
  printf("%ld plans, %d failures\n", plans, failures);
  return failures != 0;
}
