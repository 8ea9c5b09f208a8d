// bpr_vstream_scored.hip — the batched STREAM kernel with the scored samplers (bpr_vstream.h: k_vstream's SCORED
// branch; bpr_scored.h: the draw): dynamic negatives and the WARP objective under every optimizer kind, for
// bpr_train_stream_batched_scored.  A translation unit of its own, as bpr_hotlds.hip is for k_stream's LDS tier: the
// instantiations — two kinds x five optimizers x DIRECT x BIAS at six widths, the staged seen list only — compile
// beside bpr_vstream.o instead of behind it, and bpr_vstream.o's kernels stay what they were.  The checks, vs_enter,
// the DIRECT decision and the launch geometry are bpr_vstream.hip's (train_stream_batched_impl, launch_vstream).
#include <type_traits>

#include "bpr_host.h"
#define BPR_VSTREAM_KERNEL_ONLY
#include "bpr_vstream.h"

namespace bpr {

int launch_vstream_scored(bpr_ctx* c, const VStreamArgs& a, int sampler, unsigned grid, unsigned block, size_t shmem) {
  return dispatch_ge(c->G, c->E, [&](auto tag) -> int {
    using T = decltype(tag);
    constexpr int G = T::G, E = T::E;
    using std::integral_constant;
    auto go = [&](auto smp, auto knd) {
      constexpr int SMP = decltype(smp)::value, KND = decltype(knd)::value;
      auto with_bias = [&](auto dir) {
        constexpr bool DIR = decltype(dir)::value;
        if (a.Q.b != nullptr)
          hipLaunchKernelGGL((k_vstream<G, E, SMP, SEEN_LIST, KND, DIR, true>), dim3(grid), dim3(block), shmem,
                             c->stream, a);
        else
          hipLaunchKernelGGL((k_vstream<G, E, SMP, SEEN_LIST, KND, DIR, false>), dim3(grid), dim3(block), shmem,
                             c->stream, a);
      };
      if (a.alone != nullptr) with_bias(integral_constant<bool, true>{});
      else with_bias(integral_constant<bool, false>{});
    };
    auto with_kind = [&](auto smp) {
      switch (c->opt_kind) {
        case BPR_OPT_SGD: go(smp, integral_constant<int, OPT_SGD>{}); break;
        case BPR_OPT_MOMENTUM: go(smp, integral_constant<int, OPT_MOMENTUM>{}); break;
        case BPR_OPT_ADAM: go(smp, integral_constant<int, OPT_ADAM>{}); break;
        case BPR_OPT_ADAGRAD: go(smp, integral_constant<int, OPT_ADAGRAD>{}); break;
        default: go(smp, integral_constant<int, OPT_RMSPROP>{});
      }
    };
    if (sampler == NEG_WARP) with_kind(integral_constant<int, NEG_WARP>{});
    else with_kind(integral_constant<int, NEG_DYNAMIC>{});
    BPR_HIP_CHECK(hipGetLastError());
    return BPR_OK;
  });
}

}  // namespace bpr
