// bpr_opt_plan.h — the argument checks of bpr_set_optimizer and the host-side scalars of the optimizer kinds that need
// none of the lazy-replay machinery (Adagrad).  Plain C++17: no HIP, no bpr_ctx (tests/adagrad_plan_check.cpp pins it on
// the CPU under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../../include/bprcore.h"

namespace bpr {

// NULL: the kind and its hyper-parameters are accepted; else the message bpr_set_optimizer fails with
// (BPR_ERR_INVALID).  Checked before the ctx is looked at, so a refusal needs no device.
inline const char* opt_params_error(int32_t kind, const bpr_opt_params* p) {
  if (p == nullptr) return "bpr_set_optimizer: NULL argument";
  if (kind < BPR_OPT_SGD || kind > BPR_OPT_ADAGRAD) return "bpr_set_optimizer: unknown optimizer kind";
  if ((kind == BPR_OPT_MOMENTUM || kind == BPR_OPT_RMSPROP) && !(p->momentum >= 0.f && p->momentum < 1.f))
    return "bpr_set_optimizer: momentum must be in [0, 1)";
  if (!(p->lr_decay >= 0.f)) return "bpr_set_optimizer: lr_decay must be >= 0";
  if (p->lr_decay != 0.f && kind != BPR_OPT_ADAGRAD)
    return "bpr_set_optimizer: lr_decay belongs to BPR_OPT_ADAGRAD (0 for every other kind)";
  return nullptr;
}

// The kinds whose dense zero-gradient step is NO step: nothing to replay, nothing to flush, no per-row "last step".
// (SGD: w - lr * 0.  Adagrad: sum + 0 * 0, w - clr * 0 / (sqrt(sum) + eps).)
inline bool opt_kind_lazy(int32_t kind) { return kind != BPR_OPT_SGD && kind != BPR_OPT_ADAGRAD; }

// torch.optim.Adagrad's decayed rate of the 1-based step t: clr = lr / (1 + (t - 1) * lr_decay), in double, rounded
// to float once (torch computes it on Python floats and hands it to the fp32 kernel as a scalar).
inline float adagrad_clr(float lr, float lr_decay, int64_t t) {
  return (float)((double)lr / (1.0 + (double)(t - 1) * (double)lr_decay));
}

}  // namespace bpr
