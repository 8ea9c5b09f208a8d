// A stand-alone host program over revisit-bpr_amd/csrc/bpr_opt_plan.h: tests/test_adagrad_model_cpu.py compiles it with
// the host compiler under -fsanitize=address,undefined and runs it.  It holds the argument checks of bpr_set_optimizer
// (every kind, the new one included; lr_decay only with Adagrad and never negative; the momentum range as before),
// which kinds need the lazy replay, and the decayed rate against a restatement in double.  Exit status 0: all held.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "bpr_opt_plan.h"

using namespace bpr;

static int failures = 0;
#define CHECK(c)                                    \
  do {                                              \
    if (!(c)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #c); \
      ++failures;                                   \
    }                                               \
  } while (0)

static bpr_opt_params params() {
  bpr_opt_params p;
  memset(&p, 0, sizeof(p));
  p.lr = 0.05f; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-10f; p.alpha = 0.99f;
  return p;
}

static bool says(const char* msg, const char* what) { return msg != nullptr && strstr(msg, what) != nullptr; }

int main() {
  static_assert(BPR_OPT_ADAGRAD == 4, "the ABI's number of the kind");
  static_assert(sizeof(bpr_opt_params) == 36, "lr_decay is the ninth 4-byte field");
  long checks = 0;
  // ---- kinds
  for (int kind = -3; kind <= 8; ++kind) {
    const bpr_opt_params p = params();
    const char* msg = opt_params_error(kind, &p);
    ++checks;
    if (kind >= 0 && kind <= 4) CHECK(msg == nullptr);
    else CHECK(says(msg, "unknown optimizer kind"));
  }
  CHECK(says(opt_params_error(BPR_OPT_ADAGRAD, nullptr), "NULL"));
  // ---- lr_decay: Adagrad only, never negative, never NaN
  for (int kind = 0; kind <= 4; ++kind)
    for (float ld : {0.f, 1e-6f, 0.1f, 5.f, -1e-6f, -1.f, NAN, INFINITY}) {
      bpr_opt_params p = params();
      p.lr_decay = ld;
      const char* msg = opt_params_error(kind, &p);
      ++checks;
      if (!(ld >= 0.f)) CHECK(says(msg, "lr_decay must be >= 0"));
      else if (ld != 0.f && kind != BPR_OPT_ADAGRAD) CHECK(says(msg, "belongs to BPR_OPT_ADAGRAD"));
      else CHECK(msg == nullptr);
    }
  // ---- the momentum range, as before
  for (int kind = 0; kind <= 4; ++kind)
    for (float mu : {-0.1f, 0.f, 0.5f, 1.f, NAN}) {
      bpr_opt_params p = params();
      p.momentum = mu;
      const bool checked = kind == BPR_OPT_MOMENTUM || kind == BPR_OPT_RMSPROP;
      ++checks;
      CHECK((opt_params_error(kind, &p) != nullptr) == (checked && !(mu >= 0.f && mu < 1.f)));
    }
  // ---- which kinds replay
  CHECK(!opt_kind_lazy(BPR_OPT_SGD) && !opt_kind_lazy(BPR_OPT_ADAGRAD));
  CHECK(opt_kind_lazy(BPR_OPT_MOMENTUM) && opt_kind_lazy(BPR_OPT_ADAM) && opt_kind_lazy(BPR_OPT_RMSPROP));
  // ---- clr: 1-based t, in double, rounded once
  for (float lr : {0.05f, 0.001f, 1.f})
    for (float ld : {0.f, 0.05f, 0.1f, 3.f})
      for (int64_t t : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)1000, (int64_t)2000000000}) {
        const float got = adagrad_clr(lr, ld, t);
        const float want = (float)((double)lr / (1.0 + (double)(t - 1) * (double)ld));
        ++checks;
        CHECK(got == want);
        if (t == 1 || ld == 0.f) CHECK(got == lr);           // the first step takes the full rate
        if (ld > 0.f && t > 1) CHECK(got < lr && got > 0.f);  // (a 0-based t would give lr at t = 2 ...)
      }
  CHECK(adagrad_clr(0.05f, 0.05f, 2) == (float)((double)0.05f / (1.0 + (double)0.05f)));
  printf("%ld checks, %d failures\n", checks, failures);
  return failures != 0;
}
