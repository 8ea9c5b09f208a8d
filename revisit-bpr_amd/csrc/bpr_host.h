// bpr_host.h — host-side helpers shared by the translation units of libbprcore.
#pragma once
#include <stdlib.h>

#include <string>

#include "bpr_ctx.h"
#include "bpr_opt.h"

namespace bpr {

// bprcore.hip: the error string, the checks every entry point shares, the device view of the optimizer
int fail(int code, const std::string& msg);                 // sets bpr_last_error, returns code
OptDev opt_dev(const bpr_ctx* c, int64_t t);                // device view of the ctx's optimizer
int check_bound(bpr_ctx* c, const char* who, bool whole_table = true);  // tables bound? (+ folds hot deltas an async cut left)
int check_opt_state(const bpr_ctx* c, const char* who);     // state tensors the kind needs bound?
int check_triples(bpr_ctx* c, const char* who, const int32_t* users, const int32_t* pos, int64_t B,
                  bool whole_table = true);
int check_sampler(const bpr_ctx* c, const char* who, int32_t sampler, float adaptive_p,
                  const int32_t* neg, int64_t B);
// the scored samplers (sampler_scored, bpr_scored_plan.h) off plain-SGD bpr_train_stream: refused by name
int refuse_scored(const std::string& who, int32_t sampler);
float inv_log1mp(float p);
int strict_flush_impl(bpr_ctx* c);                          // STRICT lazy-replay flush (bpr_strict.hip)
void free_strict_scratch(bpr_ctx* c);                       // bpr_strict.hip
int sum_partials(bpr_ctx* c, const float* partials, int n_blocks, float* out);  // bpr_stream_launch.hip: k_sum_partials
int vs_flush(bpr_ctx* c, bool users, bool items);           // bpr_vstream.hip
int vs_leave(bpr_ctx* c);                                   // bpr_vstream.hip
void vs_free(bpr_ctx* c);                                   // bpr_vstream.hip
void comm_free(bpr_ctx* c, bool tables_alive);              // bpr_comm.hip
int comm_world(const bpr_ctx* c);                           // bpr_comm.hip (1 without a communicator)
int comm_rank(const bpr_ctx* c);
int comm_gather_snapshot(bpr_ctx* c, int32_t* order_back, float* sigma_back, int per);  // bpr_comm.hip

inline int max_blocks() {
  static int v = [] {
    const char* e = getenv("BPR_MAX_BLOCKS");
    int n = e ? atoi(e) : 0;
    return n > 0 ? n : 256 * 8;  // 256 CUs x 8 resident 256-thread blocks
  }();
  return v;
}

// grid for n groups of G lanes, 256-thread blocks, capped (grid-stride inside the kernels)
inline unsigned grid_for(int64_t n_groups, int G, int64_t cap_groups) {
  if (cap_groups > 0 && n_groups > cap_groups) n_groups = cap_groups;
  const int64_t per_block = 256 / G;
  int64_t blocks = (n_groups + per_block - 1) / per_block;
  if (blocks > max_blocks()) blocks = max_blocks();
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// ---- (G, E) dispatch: G lanes per triple, E elements per lane (bpr_device.h) --------------------
template <int A, int B>
struct GE {
  static constexpr int G = A;
  static constexpr int E = B;
};

template <typename F>
inline int dispatch_ge(int G, int E, F&& f) {
  switch (G * 32 + E) {
    case 32 * 32 + 1: return f(GE<32, 1>{});
    case 32 * 32 + 2: return f(GE<32, 2>{});
    case 32 * 32 + 4: return f(GE<32, 4>{});
    case 64 * 32 + 4: return f(GE<64, 4>{});
    case 64 * 32 + 8: return f(GE<64, 8>{});
    case 64 * 32 + 16: return f(GE<64, 16>{});
    default: return fail(BPR_ERR_UNSUPPORTED, "unsupported embedding dim");
  }
}

// bpr_hotlds.hip: k_stream with the LDS tier of the hot block, launched as the plan (bpr_stream_plan.h) says
struct StreamArgs;
struct StreamPlan;
int launch_stream_lds(bpr_ctx* c, const StreamArgs& a, int sampler, const StreamPlan& p, hipEvent_t stop);
// bpr_dynamic.hip: the plain k_stream with dynamic negatives for the ctx's shape and a "seen?" structure
using StreamKernelFn = void (*)(const StreamArgs);
int stream_kernel_dynamic(const bpr_ctx* c, int seen, StreamKernelFn* out);
// bpr_warp.hip: the same for the WARP objective
int stream_kernel_warp(const bpr_ctx* c, int seen, StreamKernelFn* out);
// bpr_dynamic.hip: what bpr_sample_dynamic and bpr_sample_warp do once the call's part of the shape and of the
// kernel arguments (bpr_scored.h) is filled: the checks, the plan and the launch of k_sample_scored
struct ScoredShape;
struct ScoredWarpArgs;
int launch_sample_scored(bpr_ctx* c, const char* who, ScoredShape s, ScoredWarpArgs a);

// bpr_vstream_scored.hip: k_vstream with dynamic negatives or the WARP objective, in the launch bpr_vstream.hip laid out
struct VStreamArgs;
int launch_vstream_scored(bpr_ctx* c, const VStreamArgs& a, int sampler, unsigned grid, unsigned block, size_t shmem);

struct Timer {
  bpr_ctx* c;
  size_t slot = 0;
  bool on = false;
  Timer(bpr_ctx* ctx, bool enabled) : c(ctx) {
    if (!enabled || !c->timing) return;
    if ((c->timing_seen++ % c->timing_stride) != 0) return;  // every timing_stride-th launch
    if (c->ev_used == c->ev_start.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      c->ev_start.push_back(a);
      c->ev_stop.push_back(b);
    }
    slot = c->ev_used++;
    on = true;
    hipEventRecord(c->ev_start[slot], c->stream);
  }
  ~Timer() {
    if (on) hipEventRecord(c->ev_stop[slot], c->stream);
  }
};

}  // namespace bpr
