// bprcore.hip — what is left of the C ABI of libbprcore.so (include/bprcore.h) once every subsystem has its own file:
// the error string, the argument checks every entry point shares, the device view of the optimizer, the life of a ctx
// and what is bound to or set on it, the epoch planner's entry points (bpr_plan.hip does the work), the step counters,
// timing, stream handles and the two plan test hooks.  It launches no kernel.  The STRICT path: bpr_strict.hip; the
// STREAM launch, bpr_sync_cut and the stand-alone samplers: bpr_stream_launch.hip; the snapshot: bpr_refresh.hip; the
// hot tier: bpr_hot.hip.  The flags that make two consecutive calls correct: bpr_ctx_state.h.
#include <math.h>
#include <string.h>

#include <string>

#include "bpr_ctx_state.h"
#include "bpr_host.h"
#include "bpr_stream_plan.h"
#include "bpr_refresh_plan.h"
#include "bpr_scored_plan.h"
#include "bpr_group_shape.h"
#include "bpr_opt_plan.h"

namespace bpr {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

int check_bound(bpr_ctx* c, const char* who, bool whole_table) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": ctx is NULL");
  if (c->P == nullptr || c->Q == nullptr)
    return fail(BPR_ERR_INVALID, std::string(who) + ": tables not bound (bpr_bind_tables)");
  // every entry point sees the item table whole — but bpr_train_stream_acut itself and the calls of
  // its pipeline that never look at the table (commit; begin when the keys are already cut)
  if (whole_table && c->hot_unfolded) return hot_fold_impl(c);
  return BPR_OK;
}

OptDev opt_dev(const bpr_ctx* c, int64_t t) {
  OptDev o;
  memset(&o, 0, sizeof(o));
  o.kind = c->opt_kind;
  o.lr = c->opt.lr; o.mu = c->opt.momentum; o.damp = c->opt.dampening;
  o.nesterov = c->opt.nesterov;
  o.b1 = c->opt.beta1; o.b2 = c->opt.beta2; o.eps = c->opt.eps; o.alpha = c->opt.alpha;
  o.t = t;
  auto safe_log = [](double x) { return x > 0.0 ? log(x) : -1.0e30; };
  o.log_b1 = safe_log((double)o.b1);
  o.log_b2 = safe_log((double)o.b2);
  o.log_mu = safe_log((double)o.mu);
  o.log_alpha = safe_log((double)o.alpha);
  // Adam replay: terms decay like (b1/sqrt(b2))^s; stop once below 1e-8 of the first
  o.kmax = 0;
  o.t_sat = -1;
  o.adam_step = 0.f;
  o.adam_bc2 = 1.f;
  if (o.kind == OPT_ADAM) {
    o.adam_step = (float)((double)o.lr / (1.0 - exp((double)t * o.log_b1)));
    o.adam_bc2 = (float)sqrt(1.0 - exp((double)t * o.log_b2));
  }
  if (o.kind == OPT_ADAGRAD) o.adam_step = adagrad_clr(c->opt.lr, c->opt.lr_decay, t);  // the step's clr
  if (o.kind == OPT_ADAM && o.b1 > 0.f) {
    const double ratio = (double)o.b1 / sqrt((double)o.b2);
    o.kmax = ratio < 1.0 ? (int)ceil(log(1e-8) / log(ratio)) : 1 << 20;
    // closed-form replay (bpr_kernels.h: opt_replay_row): needs 1 - b^t to round to 1.0f for every
    // replayed t (b^t < 2^-25) and all three series ratios b1 / b2^((j+1)/2) below 1
    const bool no_closed = c->tune_adam_closed == 0;  // bpr_set_tuning("adam_closed", 0): tests compare both routes
    const double zmax = (double)o.b1 / pow((double)o.b2, 0.5 * ADAM_SERIES);
    if (!no_closed && zmax < 0.999 && o.b1 < 1.f && o.b2 > 0.f && o.b2 < 1.f) {
      const double lim = log(ldexp(1.0, -25));
      const double t1 = ceil(lim / log((double)o.b1)), t2 = ceil(lim / log((double)o.b2));
      o.t_sat = (int64_t)(t1 > t2 ? t1 : t2);  // replayed steps are s0+1 .. : s0 >= t_sat suffices
      o.sv_min = (float)((double)o.eps * pow((double)o.b2, -0.5 * o.kmax) / 0.2);
      for (int j = 0; j < ADAM_SERIES; ++j) {
        const double lz = log((double)o.b1) - 0.5 * (j + 1) * log((double)o.b2), z = exp(lz);
        o.G[j] = (float)(z * (1.0 - exp((double)o.kmax * lz)) / (1.0 - z));
        o.log2_z[j] = (float)(lz / log(2.0));
        o.zc[j] = (float)(z / (1.0 - z));
      }
    }
  }
  return o;
}

int check_opt_state(const bpr_ctx* c, const char* who) {
  const bool need_m = c->opt_kind == BPR_OPT_MOMENTUM || c->opt_kind == BPR_OPT_ADAM ||
                      (c->opt_kind == BPR_OPT_RMSPROP && c->opt.momentum > 0.f);
  const bool need_v = c->opt_kind == BPR_OPT_ADAM || c->opt_kind == BPR_OPT_RMSPROP ||
                      c->opt_kind == BPR_OPT_ADAGRAD;  // (Adagrad: v = sum, no m)
  if ((need_m && (!c->mP || !c->mQ || (c->bias && !c->mb))) ||
      (need_v && (!c->vP || !c->vQ || (c->bias && !c->vb))))
    return fail(BPR_ERR_INVALID,
                std::string(who) + ": optimizer state not bound (bpr_bind_opt_state)");
  return BPR_OK;
}

static int drain_timing(bpr_ctx* c) {
  if (c->ev_used == 0) return BPR_OK;
  BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < c->ev_used; ++k) {
    float ms = 0.f;
    BPR_HIP_CHECK(hipEventElapsedTime(&ms, c->ev_start[k], c->ev_stop[k]));
    c->timed_ms += (double)ms;
    c->timed_launches += 1;
  }
  c->ev_used = 0;
  return BPR_OK;
}

float inv_log1mp(float p) { return (float)(1.0 / log1p(-(double)p)); }


int check_triples(bpr_ctx* c, const char* who, const int32_t* users, const int32_t* pos, int64_t B,
                  bool whole_table) {
  if (int rc = check_bound(c, who, whole_table)) return rc;
  if (B < 0 || (B > 0 && (users == nullptr || pos == nullptr)))
    return fail(BPR_ERR_INVALID, std::string(who) + ": bad argument");
  return BPR_OK;
}

int refuse_scored(const std::string& who, int32_t sampler) {
  if (!sampler_scored(sampler)) return BPR_OK;
  return fail(BPR_ERR_UNSUPPORTED, who + (sampler == BPR_NEG_WARP ? ": the WARP objective is" : ": dynamic negatives are") +
                                       " fused into the plain-SGD STREAM kernel only (bpr_train_stream)");
}

int check_sampler(const bpr_ctx* c, const char* who, int32_t sampler, float adaptive_p,
                         const int32_t* neg, int64_t B) {
  if (sampler == BPR_NEG_GIVEN) {
    if (neg == nullptr && B > 0) return fail(BPR_ERR_INVALID, std::string(who) + ": neg is NULL");
    return BPR_OK;
  }
  if (sampler != BPR_NEG_UNIFORM && sampler != BPR_NEG_ADAPTIVE && !sampler_scored(sampler))
    return fail(BPR_ERR_INVALID, std::string(who) + ": unknown sampler");
  if (c->indptr == nullptr) return fail(BPR_ERR_INVALID, std::string(who) + ": seen CSR not bound");
  if (sampler == BPR_NEG_ADAPTIVE) {
    if (!c->have_snapshot)
      return fail(BPR_ERR_INVALID, std::string(who) + ": call bpr_adaptive_refresh first");
    if (!(adaptive_p > 0.f && adaptive_p < 1.f))
      return fail(BPR_ERR_INVALID, std::string(who) + ": adaptive_p not in (0,1)");
  }
  return BPR_OK;
}

}  // namespace bpr

using namespace bpr;

extern "C" {

int bpr_version(void) { return BPRCORE_VERSION; }
const char* bpr_last_error(void) { return g_last_error.c_str(); }

int bpr_ctx_create(bpr_ctx** out, int device_id, void* hip_stream) {
  if (out == nullptr) return fail(BPR_ERR_INVALID, "bpr_ctx_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(BPR_ERR_HIP, "bpr_ctx_create: no HIP device visible (libbprcore has no CPU path)");
  if (device_id < 0 || device_id >= ndev)
    return fail(BPR_ERR_INVALID, "bpr_ctx_create: bad device id");
  BPR_HIP_CHECK(hipSetDevice(device_id));
  bpr_ctx* c = new (std::nothrow) bpr_ctx();
  if (c == nullptr) return fail(BPR_ERR_NOMEM, "bpr_ctx_create: out of host memory");
  c->device = device_id;
  c->stream = (hipStream_t)hip_stream;
  if (hipMalloc(&c->dev_scalars, sizeof(float) * 2 * 4 * (size_t)(STREAM_MAX_GRID + 1)) != hipSuccess) {
    delete c;
    return fail(BPR_ERR_HIP, "bpr_ctx_create: hipMalloc failed");
  }
  *out = c;
  return BPR_OK;
}

int bpr_ctx_destroy(bpr_ctx* c) {
  if (c == nullptr) return BPR_OK;
  hipSetDevice(c->device);
  // The caller's streams may be GONE by now: a garbage collector destroys the objects of a finished
  // trainer in any order, and hipStreamSynchronize on a destroyed (CU-masked) stream aborts inside the
  // runtime ("std::system_error: Invalid argument") or hangs — the intermittent failure of the two-rank
  // parity run (r5).  So: wait for the DEVICE, and do whatever cleanup work is left on the default stream.
  hipDeviceSynchronize();
  c->stream = nullptr;
  if (!c->side_owned) c->side = nullptr;
  free_strict_scratch(c);
  comm_free(c, false);  // (no fold into tables that may be gone)
  refresh_free(c);
  side_free(c);
  vs_free(c);
  hipFree(c->bias_w);
  hipFree(c->dev_scalars);
  if (c->ev_launch) hipEventDestroy(c->ev_launch);
  for (auto e : c->ev_start) hipEventDestroy(e);
  for (auto e : c->ev_stop) hipEventDestroy(e);
  delete c;
  return BPR_OK;
}

int bpr_set_stream(bpr_ctx* c, void* hip_stream) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_stream: ctx is NULL");
  c->stream = (hipStream_t)hip_stream;
  return BPR_OK;
}

int bpr_bind_tables(bpr_ctx* c, float* P, int64_t U, float* Q, int64_t I, int32_t d,
                    float* item_bias, int32_t pad_user, int32_t pad_item) {
  if (c == nullptr || P == nullptr || Q == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: NULL argument");
  if (U < 1 || I < 2 || U >= ((int64_t)1 << 30) || I >= ((int64_t)1 << 30))
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: table sizes out of range");
  if (d < 1 || d > 1024)
    return fail(BPR_ERR_UNSUPPORTED, "bpr_bind_tables: embedding dim must be in [1, 1024]");
  if (((uintptr_t)P | (uintptr_t)Q) & 3u)
    return fail(BPR_ERR_INVALID, "bpr_bind_tables: tables must be 4-byte aligned");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->U != U || c->I != I || c->d != d) {
    BPR_HIP_CHECK(hipStreamSynchronize(c->stream));
    free_strict_scratch(c);
    refresh_free(c);
    vs_free(c);
  } else if (c->vs_active && (c->P != P || c->Q != Q || c->bias != item_bias)) {
    if (int rc = vs_leave(c)) return rc;  // pending steps belong to the tables bound so far
  }
  c->P = P; c->Q = Q; c->bias = item_bias;
  bias_moved(c);
  items_moved(c);
  c->U = U; c->I = I; c->d = d;
  c->pad_user = pad_user; c->pad_item = pad_item;
  const GroupShape g = group_shape(d);  // (bpr_group_shape.h: G = 32 up to d = 128, else 64)
  c->G = g.G;
  c->E = g.E;
  return BPR_OK;
}

int bpr_bind_seen_csr(bpr_ctx* c, const int64_t* indptr, const int32_t* indices) {
  if (c == nullptr || indptr == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_bind_seen_csr: NULL argument");
  c->indptr = indptr;
  c->indices = indices;
  c->heavy_for = nullptr;  // the heavy users' bitmaps belong to the CSR bound before: rebuilt lazily
  return BPR_OK;
}

int bpr_bind_item_weights(bpr_ctx* c, const float* accept, const int32_t* alias) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bind_item_weights: ctx is NULL");
  if ((accept == nullptr) != (alias == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_bind_item_weights: accept and alias go together");
  c->w_accept = accept;
  c->w_alias = alias;
  return BPR_OK;
}

int bpr_set_reg(bpr_ctx* c, float alpha_user, float alpha_item, float alpha_neg) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_reg: ctx is NULL");
  c->au = alpha_user; c->ai = alpha_item; c->an = alpha_neg;
  return BPR_OK;
}

int bpr_set_optimizer(bpr_ctx* c, int32_t kind, const bpr_opt_params* params) {
  // the kind and its hyper-parameters first (bpr_opt_plan.h): a refusal of those needs no ctx
  if (const char* msg = opt_params_error(kind, params)) return fail(BPR_ERR_INVALID, msg);
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_optimizer: ctx is NULL");
  if (c->vs_active && (kind != c->opt_kind || memcmp(&c->opt, params, sizeof(*params)) != 0)) {
    // batched STREAM: pending steps and the replay of missed ones use the hyper-parameters in
    // force when they were taken — bring every row to "now" before those change
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;
  }
  c->opt_kind = kind;
  c->opt = *params;
  return BPR_OK;
}

int bpr_bind_opt_state(bpr_ctx* c, float* m_P, float* v_P, float* m_Q, float* v_Q, float* m_bias,
                       float* v_bias) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bind_opt_state: ctx is NULL");
  if (c->vs_active && (c->mP != m_P || c->vP != v_P || c->mQ != m_Q || c->vQ != v_Q ||
                       c->mb != m_bias || c->vb != v_bias)) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;  // finish with the state tensors bound so far
  }
  c->mP = m_P; c->vP = v_P; c->mQ = m_Q; c->vQ = v_Q; c->mb = m_bias; c->vb = v_bias;
  return BPR_OK;
}

int bpr_stream_create(int device_id, const uint32_t* cu_mask, int32_t mask_words, void** stream_out) {
  if (stream_out == nullptr || mask_words < 0 || (mask_words > 0 && cu_mask == nullptr))
    return fail(BPR_ERR_INVALID, "bpr_stream_create: bad argument");
  BPR_HIP_CHECK(hipSetDevice(device_id));
  hipStream_t st = nullptr;
  if (mask_words == 0)
    BPR_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  else
    BPR_HIP_CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask_words, cu_mask));
  *stream_out = (void*)st;
  return BPR_OK;
}

int bpr_stream_destroy(void* hip_stream) {
  if (hip_stream == nullptr) return BPR_OK;
  BPR_HIP_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
  BPR_HIP_CHECK(hipStreamDestroy((hipStream_t)hip_stream));
  return BPR_OK;
}

int bpr_set_tuning(bpr_ctx* c, const char* key, int32_t value) {
  if (c == nullptr || key == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_tuning: NULL argument");
  const std::string k = key;
  if (k == "seen" && value >= 0 && value <= 3) c->tune_seen = value;
  else if (k == "vs_direct" && value >= -1 && value <= 1) c->tune_vs_direct = value;
  else if (k == "adam_closed" && (value == 0 || value == 1)) c->tune_adam_closed = value;
  else if (k == "partial_snapshot" && (value == 0 || value == 1)) c->tune_partial = value;
  else if (k == "binned_sort" && (value == 0 || value == 1)) c->tune_binned = value;
  else if (k == "binned_split" && value >= 0 && value <= 16) c->tune_binned_split = value;
  else if (k == "partial_target" && value >= 1 && value <= 1024) c->partial_target = value;
  else if (k == "refresh_sub" && (value == 0 || value == 1 || value == 2 || value == 4)) c->tune_refresh_sub = value;
  else if (k == "lds_block" && value >= 0 && value <= 1024 && value % 64 == 0) c->tune_lds_block = value;
  else if (k == "lds_tail" && value >= 0 && value <= 50) c->tune_lds_tail = value;
  else if (k == "plan_input_sorted" && (value == 0 || value == 1)) c->tune_plan_sorted = value;
  else if (k == "acut_fold" && (value == 0 || value == 1)) c->tune_acut_fold = value;
  else return fail(BPR_ERR_INVALID, "bpr_set_tuning: unknown key or value out of range");
  c->stream_occ.clear();
  return BPR_OK;
}

int bpr_set_bias_tracking(bpr_ctx* c, int32_t on) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_bias_tracking: ctx is NULL");
  c->bias_track = on != 0;
  bias_moved(c);  // (what the wide table holds was not tracked so far)
  return BPR_OK;
}

int bpr_bias_written(bpr_ctx* c) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_bias_written: ctx is NULL");
  bias_moved(c);
  return BPR_OK;
}

// Test hook, not API (tests/test_stream_plan_cpu.py sets its signature): the launch plan of a shape given as plain
// integers — StreamShape's fields in order — and an occupancy; out = StreamPlan's fields in order.  Needs no GPU.
int bpr_test_stream_plan(const int64_t* in, int32_t occ, int64_t* out) {
  StreamShape s = {};
  s.n = in[0]; s.I = in[1]; s.d = (int)in[2]; s.G = (int)in[3]; s.E = (int)in[4];
  s.sampler = (int)in[5]; s.cap_groups = in[6]; s.run_len = (int)in[7]; s.force_seen = (int)in[8];
  s.cus = (int)in[9]; s.grid_cap = in[10]; s.hot = in[11] != 0; s.hot_H = (int)in[12];
  s.tune_hot_lds = (int)in[13]; s.tune_hot_lds_force = in[14] != 0;
  s.tune_lds_block = (int)in[15]; s.tune_lds_tail = (int)in[16]; s.lds_allowed = in[17] != 0;
  const StreamPlan p = plan_stream(s, plan_stream_block(s), occ);
  const int64_t v[] = {p.kernel, p.seen, p.block, p.grid, (int64_t)p.shmem, p.bm_words, p.gpw_active, p.run_len,
                       p.L, p.tail1, p.tail2};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}

// Test hook, not API (tests/test_refresh_plan_cpu.py sets its signature): the sorter plan of a refresh given as plain
// integers — RefreshShape's fields in order; out = RefreshPlan's fields in order.  Needs no GPU.
int bpr_test_refresh_plan(const int64_t* in, int64_t* out) {
  RefreshShape s = {};
  s.I = in[0]; s.nf = (int)in[1]; s.split = in[2] != 0; s.part = in[3] != 0;
  s.tune_binned = (int)in[4]; s.tune_binned_split = (int)in[5]; s.tune_refresh_sub = (int)in[6];
  s.tune_partial = (int)in[7]; s.no_fast = in[8] != 0;
  const RefreshPlan p = plan_refresh(s);
  const int64_t v[] = {p.route, p.sub, p.len, p.g, p.sitems, p.items, p.fallback, p.fb_items, p.wide, p.partial};
  memcpy(out, v, sizeof(v));
  return BPR_OK;
}

int bpr_set_stream_opts(bpr_ctx* c, int32_t grouped_by_user, int32_t run_len) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_set_stream_opts: ctx is NULL");
  if (run_len < 0 || run_len > 30)
    return fail(BPR_ERR_INVALID, "bpr_set_stream_opts: run_len must be 0 (by launch size) or in [1, 30] (one lane of a "
                                 "32-lane group per triple of the run, plus two neighbours)");
  c->grouped = grouped_by_user != 0;
  c->run_len = run_len;
  return BPR_OK;
}

int bpr_plan_epoch(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n,
                   int64_t chunk, uint64_t seed, int32_t* users_out, int32_t* pos_out) {
  if (int rc = check_bound(c, "bpr_plan_epoch")) return rc;
  if (n < 0 || chunk < 1 || (n > 0 && (!users_in || !pos_in || !users_out || !pos_out)))
    return fail(BPR_ERR_INVALID, "bpr_plan_epoch: bad argument");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  return plan_epoch_impl(c, users_in, pos_in, n, chunk, seed, users_out, pos_out);
}

int bpr_plan_chunk(bpr_ctx* c, const int32_t* users_in, const int32_t* pos_in, int64_t n, int64_t chunk,
                   uint64_t seed, int64_t index, int32_t* users_out, int32_t* pos_out, int32_t on_side) {
  if (int rc = check_bound(c, "bpr_plan_chunk")) return rc;
  if (n < 1 || n >= ((int64_t)1 << 31) || chunk < 1 || index < 0 || !users_in || !pos_in || !users_out ||
      !pos_out)
    return fail(BPR_ERR_INVALID, "bpr_plan_chunk: bad argument");
  BPR_HIP_CHECK(hipSetDevice(c->device));
  if (c->hot_key_ptr != pos_in || c->hot_key_n != n) {  // new training set: measure popularity (as
    if (int rc = hot_build_impl(c, pos_in, n)) return rc;  // bpr_plan_epoch does)
  }
  if (!on_side) return plan_chunk_impl(c, users_in, pos_in, n, chunk, seed, index, users_out, pos_out, c->stream);
  // behind the split refresh's sort on the side stream; what bpr_adaptive_refresh_commit waits for
  // then covers this chunk too (one event, no extra packet on the launch stream)
  if (c->side == nullptr || !c->refresh_pending)
    return fail(BPR_ERR_INVALID, "bpr_plan_chunk: on_side needs a split refresh in flight "
                                 "(bpr_adaptive_refresh_begin first)");
  if (int rc = plan_chunk_impl(c, users_in, pos_in, n, chunk, seed, index, users_out, pos_out, c->side))
    return rc;
  BPR_HIP_CHECK(hipEventRecord(c->ev_sorted, c->side));
  return BPR_OK;
}

int bpr_get_step_host(bpr_ctx* c, int64_t* step_host) {
  if (c == nullptr || step_host == nullptr)
    return fail(BPR_ERR_INVALID, "bpr_get_step_host: NULL argument");
  *step_host = c->step;
  return BPR_OK;
}

int bpr_set_step(bpr_ctx* c, int64_t step) {
  if (c == nullptr || step < 0) return fail(BPR_ERR_INVALID, "bpr_set_step: bad argument");
  if (c->vs_active) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    if (int rc = vs_leave(c)) return rc;
  }
  // rows are assumed flushed at `step` (a checkpoint is written after bpr_flush_lazy)
  c->step = step;
  if (c->lastP != nullptr) {
    BPR_HIP_CHECK(hipSetDevice(c->device));
    BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastP, (int)step, (size_t)c->U, c->stream));
    BPR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)c->lastQ, (int)step, (size_t)c->I, c->stream));
  }
  return BPR_OK;
}

int bpr_set_sampler_iter(bpr_ctx* c, int64_t iteration) {
  if (c == nullptr || iteration < 0)
    return fail(BPR_ERR_INVALID, "bpr_set_sampler_iter: bad argument");
  c->strict_iter = iteration;
  return BPR_OK;
}

int bpr_timing_enable(bpr_ctx* c, int32_t on) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_timing_enable: ctx is NULL");
  if (int rc = drain_timing(c)) return rc;
  c->timing = on != 0;
  c->timing_stride = on > 1 ? on : 1;
  c->timing_seen = 0;
  c->timed_ms = 0.0;
  c->timed_launches = 0;
  return BPR_OK;
}

int bpr_timing_read_host(bpr_ctx* c, double* avg_ms_host, int64_t* launches_host) {
  if (c == nullptr) return fail(BPR_ERR_INVALID, "bpr_timing_read_host: ctx is NULL");
  if (int rc = drain_timing(c)) return rc;
  if (avg_ms_host) *avg_ms_host = c->timed_launches ? c->timed_ms / (double)c->timed_launches : 0.0;
  if (launches_host) *launches_host = c->timed_launches;
  return BPR_OK;
}

}  // extern "C"
