/*
 * bprcore.h — C ABI of libbprcore.so, the MI355X (gfx950) BPR-MF training engine.
 *
 * The reference (Nemexur/revisit-bpr) has no FFI: its hot path is a chain of stock torch ops
 * called from Python.  Each entry point below therefore cites the reference *Python call site*
 * it replaces (paths relative to the reference tree).  The binding a maintainer adds on the
 * reference side is a ctypes stub — see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, no exceptions across the boundary.
 *   - Every pointer argument is a DEVICE pointer (HBM) unless the name ends in `_host`.
 *   - The caller owns every buffer it passes in.  The library allocates only private scratch
 *     inside `bpr_ctx` (grad accumulators of the strict path, adaptive-sampler order arrays,
 *     scalar reduction slots) and frees it in bpr_ctx_destroy.
 *   - Return value: 0 (BPR_OK) on success, negative bpr_status on failure; the message for the
 *     calling thread is available from bpr_last_error().  The library never aborts.
 *   - All calls are asynchronous with respect to the host and are ordered on the HIP stream the
 *     ctx was created with (pass torch's current stream) — except bpr_ctx_create/destroy and the
 *     `*_host` getters, which synchronise that stream.
 *   - A ctx is single-threaded and tied to one HIP device + stream.
 *   - Embedding dim d in [1, 1024]; tables row-major fp32, 4-byte aligned.
 *   - Row 0 of both tables is the pad row (reference: nn.Embedding(padding_idx=0)); item ids
 *     handed to the library are in [0, I), user ids in [0, U).  Ids are int32.
 */
#ifndef BPRCORE_H
#define BPRCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPRCORE_VERSION 100 /* 0.1.0 */

typedef struct bpr_ctx bpr_ctx;

typedef enum bpr_status {
  BPR_OK = 0,
  BPR_ERR_INVALID = -1,     /* bad argument / state (message says which) */
  BPR_ERR_HIP = -2,         /* a HIP runtime call failed */
  BPR_ERR_UNSUPPORTED = -3, /* valid request the engine does not implement (e.g. d > 1024) */
  BPR_ERR_NOMEM = -4
} bpr_status;

/* torch.optim.* kinds used by the reference configs
 * (configs/RQ1/ours.yaml.j2:116-119, configs/RQ2/optimizers/, configs/RQ3/time-split/ada-sampling-adam.yaml.j2:169-175) */
typedef enum bpr_opt_kind {
  BPR_OPT_SGD = 0,      /* torch.optim.SGD(lr)                               */
  BPR_OPT_MOMENTUM = 1, /* torch.optim.SGD(lr, momentum, dampening, nesterov) */
  BPR_OPT_ADAM = 2,     /* torch.optim.Adam(lr, betas, eps)                   */
  BPR_OPT_RMSPROP = 3,  /* torch.optim.RMSprop(lr, alpha, eps, momentum)      */
  /* Extension (not in the reference configs): sum += g * g; w -= clr * g / (sqrt(sum) + eps) in fp32 with correctly
   * rounded sqrt and divide, clr = lr / (1 + (t - 1) * lr_decay) in double, rounded once per step.  A zero gradient
   * moves neither the row nor its sum, so a dense torch.optim.Adagrad IS the row-sparse update: nothing is replayed
   * and bpr_flush_lazy / bpr_flush_items have nothing to do for it on the STRICT path.  Runs on STRICT (bpr_step,
   * bpr_apply, bpr_train_strict) and on bpr_train_stream_batched.  bpr_train_stream and its cut variants — the fused
   * k_stream, its LDS tier and the hot block — stay plain SGD and return BPR_ERR_UNSUPPORTED for this kind before
   * the device is touched: these fold linear deltas.  Adagrad's step is not linear. */
  BPR_OPT_ADAGRAD = 4   /* torch.optim.Adagrad(lr, lr_decay, eps) */
} bpr_opt_kind;

typedef struct bpr_opt_params {
  float lr;
  float momentum;  /* MOMENTUM; RMSPROP (0 = none) */
  float dampening; /* MOMENTUM */
  int32_t nesterov;
  float beta1, beta2; /* ADAM */
  float eps;          /* ADAM (1e-8), RMSPROP (1e-8), ADAGRAD (torch's default: 1e-10) */
  float alpha;        /* RMSPROP smoothing constant (0.99) */
  float lr_decay;     /* ADAGRAD (0 = no decay); must be 0 for every other kind */
} bpr_opt_params;

/* How a step treats rows that occur several times in the same batch / chunk. */
typedef enum bpr_mode {
  /* Exact reference mini-batch semantics (revisit_bpr/models/bpr/model.py:40-68 + trainer.py:76-81):
   * all B gradients evaluated at the pre-step parameters, duplicates accumulated, ONE optimizer
   * step.  Two kernels (grad-accumulate, apply).  Launch-bound at B=256; used for parity. */
  BPR_MODE_STRICT = 0,
  /* Throughput path: one launch consumes a whole chunk of triples; every triple reads the latest
   * rows it can see and applies its update immediately with per-element fp32 atomics
   * (asynchronous SGD, bounded staleness).  SGD only; the other optimizers (BPR_OPT_ADAGRAD included) have their
   * own single-launch path, bpr_train_stream_batched. */
  BPR_MODE_STREAM = 1
} bpr_mode;

typedef enum bpr_sampler_kind {
  BPR_NEG_GIVEN = 0,   /* caller passes `neg` */
  BPR_NEG_UNIFORM = 1, /* revisit_bpr/modules/neg_samplers.py:31-37 (UniformSampler.sample) */
  BPR_NEG_ADAPTIVE = 2, /* revisit_bpr/modules/neg_samplers.py:74-124 (AdaptiveSampler.sample) */
  /* Dynamic negative sampling (extension; Zhang et al., SIGIR 2013): the highest-scoring of M unseen uniform
   * candidates under the model as it is now (bpr_set_dynamic, bpr_sample_dynamic).  Accepted by bpr_train_stream /
   * _cut (plain SGD); bpr_train_stream_acut, bpr_train_strict, bpr_train_stream_batched, the STRICT mode of bpr_step
   * and the other fold-in entry points return BPR_ERR_UNSUPPORTED for it before the device is touched: draw with
   * bpr_sample_dynamic and pass the picks as BPR_NEG_GIVEN there.  bpr_fold_in_rows_scored folds users in with it;
   * bpr_train_stream_batched_scored is the batched STREAM launch with it, under any optimizer kind. */
  BPR_NEG_DYNAMIC = 3,
  /* The WARP objective (extension; Weston, Bengio, Usunier, IJCAI 2011 — LightFM's default loss): not a sampler of
   * negatives for BPR's log-sigmoid loss but another pairwise loss, chosen here because it replaces the draw AND the
   * step's weight: the first of N unseen uniform candidates that comes within `margin` of the positive's score, a
   * step weighted by log(estimated rank), no step when nothing violates (bpr_set_warp, bpr_sample_warp).  Accepted
   * and refused exactly where BPR_NEG_DYNAMIC is: bpr_train_stream / _cut and STREAM-mode bpr_step (plain SGD) run
   * it; bpr_train_stream_acut, bpr_train_strict, bpr_train_stream_batched, the STRICT mode of bpr_step and the
   * other fold-in entry points return BPR_ERR_UNSUPPORTED for it before the device is touched;
   * bpr_fold_in_rows_scored folds users in with it, bpr_train_stream_batched_scored is the batched STREAM launch with
   * it, under any optimizer kind. */
  BPR_NEG_WARP = 4
} bpr_sampler_kind;

/* out_scalars layout written by bpr_forward_grad / bpr_step / bpr_train_stream (fp32, ADDED to —
 * zero it first):  [0] bpr_loss = Σ −logσ(x)   [1] l2_reg   [2] Σ|x|   [3] number of triples */
#define BPR_SCALARS 4

/* ---- lifecycle ------------------------------------------------------------------------- */
int bpr_version(void);
const char* bpr_last_error(void);
/* hip_stream: a hipStream_t (may be NULL = default stream). */
int bpr_ctx_create(bpr_ctx** out, int device_id, void* hip_stream);
int bpr_ctx_destroy(bpr_ctx* ctx);
int bpr_set_stream(bpr_ctx* ctx, void* hip_stream);

/* ---- model state (reference: MF parameters, revisit_bpr/models/bpr/model.py:97-116) ------ */
/* P [U,d], Q [I,d] row-major fp32, updated IN PLACE; item_bias [I] or NULL (MF(item_bias=...)).
 * pad_user / pad_item: the nn.Embedding padding_idx of each table (−1 = none): gradient of that
 * embedding row is dropped, as torch's embedding backward does. */
int bpr_bind_tables(bpr_ctx* ctx, float* P, int64_t U, float* Q, int64_t I, int32_t d,
                    float* item_bias, int32_t pad_user, int32_t pad_item);

/* Seen-items CSR over users: indptr [U+1] int64, indices [nnz] int32 sorted ascending inside each
 * row, no duplicates, no item 0.  Replaces the padded `seen_items` [B,S] batch tensor
 * (experiments/bpr/dataset.py:142-190, example.py:33-68) for on-device sampling.  The first
 * sampling STREAM launch after a bind derives private scratch from it (I-bit seen bitmaps in HBM
 * for users with more than 256 seen items: one-time, synchronous): bind again after changing the
 * arrays' contents. */
int bpr_bind_seen_csr(bpr_ctx* ctx, const int64_t* indptr, const int32_t* indices);

/* Model.regularization alphas after the resolution rules of model.py:74-86 were applied by the host. */
int bpr_set_reg(bpr_ctx* ctx, float alpha_user, float alpha_item, float alpha_neg);

/* torch.optim hyper-parameters (read from optimizer.param_groups by the host shim each step).  The kind and its
 * hyper-parameters are checked before the ctx is looked at: an unknown kind, a momentum outside [0, 1), lr_decay < 0
 * (or NaN) and a non-zero lr_decay with any kind but BPR_OPT_ADAGRAD are BPR_ERR_INVALID. */
int bpr_set_optimizer(bpr_ctx* ctx, int32_t kind, const bpr_opt_params* params);
/* Optimizer state, same shapes as the tables (caller-owned so checkpoints keep working):
 *   MOMENTUM: m_* = momentum_buffer;  ADAM: m_* = exp_avg, v_* = exp_avg_sq;  RMSPROP: v_* = square_avg
 *   (+ m_* = momentum_buffer when momentum > 0);  ADAGRAD: v_* = sum (m_* may be NULL: never read or written).
 * *_bias may be NULL when there is no item_bias.  All zero-initialised by the caller — except Adagrad's sum, which
 * the caller fills with torch's initial_accumulator_value (0 by default): the library only ever adds to it. */
int bpr_bind_opt_state(bpr_ctx* ctx, float* m_P, float* v_P, float* m_Q, float* v_Q,
                       float* m_bias, float* v_bias);

/* ---- negative sampling -------------------------------------------------------------------- */
/* Draw one negative per (user) uniformly over items the user has not seen, never item 0.
 * Randomness: Philox4x32-10 keyed by `seed`, counter = offset + position in the batch, so a triple's
 * negative does not depend on launch geometry or GPU count.  neg_out [B] int32. */
int bpr_sample_uniform(bpr_ctx* ctx, const int32_t* users, int64_t B, uint64_t seed,
                       uint64_t offset, int32_t* neg_out);

/* Dynamic negative sampling.  For the triple with counter t = offset + position, user u and M candidates:
 *   candidates   bpr_sample_uniform's stream for (seed, t), item weights included: candidate k = 0 .. 4,095;
 *   accepted     the candidates u has not seen; a_1 .. a_m = the first min(M, accepted) of them in order of k
 *                (drawn with replacement: duplicates stay);
 *   none         if none of the 4,096 is accepted the result is bpr_sample_uniform's (its exact pick by rank; item 0
 *                when nothing is unseen);
 *   score(a)     <P[u], Q[a]> (+ item_bias[a]) in fp32, on the rows as the kernel sees them;
 *   pick         best = a_1; for i = 2 .. m: a_i replaces best if score(a_i) > score(best), or if score(best) is NaN
 *                and score(a_i) is not.  Equal scores keep the earlier candidate, an all-NaN set keeps a_1.
 * So M = 1 IS bpr_sample_uniform, and so is any M when all scores are equal.
 * bpr_set_dynamic: M of the ctx's STREAM launches with BPR_NEG_DYNAMIC, 1 .. 32 (else BPR_ERR_INVALID), default 4 —
 * a parameter of the method, not a bpr_set_tuning key.
 * bpr_sample_dynamic: the stand-alone kernel, one draw per entry of users [B] from the ctx's tables, item_bias, seen
 * CSR and item weights as they are in stream order; neg_out [B] int32, score_out [B] fp32 or NULL = the picks'
 * scores.  It reduces a score in the order the STREAM kernel does at the ctx's embedding width, so on tables that do
 * not move its picks are that kernel's, bit for bit.  candidates outside 1 .. 32, users or neg_out NULL, B < 0, no
 * seen CSR: BPR_ERR_INVALID, nothing launched.  The rows are read as stored: with a stateful optimizer on the STRICT
 * path call bpr_flush_lazy first. */
int bpr_set_dynamic(bpr_ctx* ctx, int32_t candidates);
int bpr_sample_dynamic(bpr_ctx* ctx, const int32_t* users, int64_t B, int32_t candidates, uint64_t seed,
                       uint64_t offset, int32_t* neg_out, float* score_out /* may be NULL */);

/* The WARP objective.  For the triple with counter t = offset + position, user u, positive i, N = max_sampled:
 *   candidates   bpr_sample_dynamic's: a_1 .. a_m = the first min(N, accepted) unseen candidates of
 *                bpr_sample_uniform's stream for (seed, t) in order, item weights included, duplicates kept; if none
 *                of the 4,096 is accepted, a_1 = bpr_sample_uniform's exact pick by rank (item 0 when nothing is unseen);
 *   scores       x_i = <P[u], Q[i]> (+ item_bias[i]), x_k = <P[u], Q[a_k]> (+ item_bias[a_k]) in fp32, on the rows as
 *                the kernel sees them;
 *   violator     the smallest k with x_k > x_i - margin (a NaN on either side compares false: a NaN candidate never
 *                violates, a NaN positive skips the triple); tries = k;
 *   skipped      no k in 1 .. m violates: no step of any kind, nothing written, nothing added to the loss scalars;
 *   weight       L = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - |seen(u)|, not clipped; L may be 0;
 *   step         bpr_train_stream's plain-SGD step on (u, i, a_k) with L in the place of sigma(-x): the L2 terms, lr,
 *                item_bias handling and hot block are the same (L = 0: the L2 terms alone);
 *   scalars      slot 0 (the BPR-loss slot) carries sum L (margin - x_i + x_k), slot 1 the L2 term, slot 2 sum
 *                |x_i - x_k|, slot 3 the count — all over the stepped triples only.
 * N = 1 on a user whose every unseen item violates IS bpr_sample_uniform.
 * bpr_set_warp: (max_sampled, margin) of the ctx's STREAM launches with BPR_NEG_WARP; max_sampled in 1 .. 32, margin
 * finite and > 0 (else BPR_ERR_INVALID); default (10, 1.0f) — 10 is LightFM's max_sampled.
 * bpr_sample_warp: the stand-alone kernel, one draw per entry of users / pos [n] from the ctx's tables, item_bias,
 * seen CSR and item weights as they are in stream order.  neg_out [n] int32: the violator, -1 = skipped; tries_out
 * [n] int32: k, 0 = skipped; xpos_out / xneg_out [n] fp32 or NULL: x_i and the violator's x_k (0 when skipped).  It
 * reduces a score in the order the STREAM kernel does at the ctx's embedding width, so on tables that do not move its
 * picks are that kernel's, bit for bit.  Bad max_sampled or margin, users / pos / neg_out / tries_out NULL, n < 0, no
 * seen CSR: BPR_ERR_INVALID, nothing launched. */
int bpr_set_warp(bpr_ctx* ctx, int32_t max_sampled, float margin);
int bpr_sample_warp(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int64_t n, int32_t max_sampled,
                    float margin, uint64_t seed, uint64_t offset, int32_t* neg_out, int32_t* tries_out,
                    float* xpos_out /* may be NULL */, float* xneg_out /* may be NULL */);

/* Item weights of the uniform sampler — BPRExperiment._static_sampling with
 * item_counts ** neg_sampling_alpha (experiments/bpr/exp.py:85-91, 282-293): P(negative = i) =
 * w_i / (sum of w over the user's unseen items), w_0 = 0.  The caller passes a Walker alias table
 * over items 1..I-1 (accept [I] fp32, alias [I] int32, entry 0 unused; the host shim builds it):
 * candidate = column c if frac(r (I-1) / 2^32) < accept[c] else alias[c]; seen candidates are
 * rejected as before.  NULL, NULL = uniform (the default).  Affects every uniform draw of the ctx
 * (bpr_sample_uniform, bpr_step, bpr_train_*).
 * Deviation: when 4,096 candidates in a row were all seen (a user who has seen nearly every item)
 * the exact fallback picks by rank UNIFORMLY among the user's unseen items — it does not carry the
 * weights, the reference's multinomial over the masked weights would (neg_samplers.py:31-37).  The
 * oracle restates the same rule; the chance of reaching the fallback is (seen weight share)^4096. */
int bpr_bind_item_weights(bpr_ctx* ctx, const float* accept, const int32_t* alias);

/* AdaptiveSampler.update_stats (neg_samplers.py:126-132): snapshot the item table as per-factor
 * descending item orders (private scratch, d*I int32) and sigma_f = unbiased std over rows 1..
 * The sorter goes by the table's size (csrc/bpr_refresh_plan.h): 2,048 .. 20,480 items the binned sort with one
 * workgroup per column, up to 131,071 items with several (16-bit ids to 65,535 items, 17-bit ids beyond — Yelp's
 * 92,090), otherwise and below the in-LDS radix sort (+ merge of 2 | 4 runs up to 147,456 items), beyond that a
 * device-wide radix sort; every route gives the same stable order, bit for bit. */
int bpr_adaptive_refresh(bpr_ctx* ctx);
/* What the last COMPLETED refresh ran (bpr_adaptive_refresh, _commit or _publish; a split refresh still pending
 * does not count) — a diagnostic, never on the training path: it waits for the ctx stream.  info_host: HOST
 * array of BPR_REFRESH_INFO_LEN int32, every entry -1 before the first refresh:
 *   [0] route  0 in-LDS radix sort (+ merge of sub runs) | 1 binned sort, one workgroup per column |
 *              2 split binned sort, G workgroups per column | 3 partial order | 4 device-wide radix sort
 *   [1] G      workgroups per column of the binned sort (0 when the route is not a binned one)
 *   [2] ITEMS  keys per thread of the route's kernel instantiation (SITEMS of the split binned sort; 0 for route 4)
 *   [3] sub    workgroups per column of the radix sort: the route's own, or the fallback's behind route 2
 *   [4] columns the split binned sort handed to its fallback (route 2; -1 on every other route, whose kernels
 *       leave no trace of it)
 *   [5..7] reserved, -1 */
#define BPR_REFRESH_INFO_LEN 8
int bpr_adaptive_refresh_info(bpr_ctx* ctx, int32_t* info_host);
/* The same refresh in two halves, so that the sort does not stand between two STREAM launches
 * (the reference sorts inline: update_stats is called from sample(), neg_samplers.py:122-123).
 * _begin: the snapshot's keys are cut from the item table NOW, in the ctx stream's order — that
 * instant is the snapshot's point in time — and their per-factor sort is queued on the ctx's SIDE
 * stream; the ctx stream does not wait, and every sampler keeps reading the previous snapshot.
 * _commit: the ctx stream waits for that sort; launches after it read the new snapshot.
 * bpr_adaptive_refresh == _begin + _commit with nothing in between.  One split refresh may be
 * pending at a time (_begin while pending: BPR_ERR_INVALID; bpr_adaptive_refresh while pending
 * is refused as well — commit first).  What the caller puts between the two calls decides the
 * snapshot's age: `commit; begin; bpr_train_stream(chunk)` per chunk makes every chunk sample from
 * the item table as it was one chunk earlier (DESIGN.md section 4.3 holds the parity evidence). */
int bpr_adaptive_refresh_begin(bpr_ctx* ctx);
int bpr_adaptive_refresh_commit(bpr_ctx* ctx);
/* *pending_host (HOST pointer) = 1 while a split refresh awaits its commit. */
int bpr_adaptive_refresh_pending(bpr_ctx* ctx, int32_t* pending_host);
/* PARTIAL snapshots (r5, opt-in: bpr_set_tuning(ctx, "partial_snapshot", 1); "partial_target" = keys aimed at
 * per exact end, 1..1024, default 640).  All the sampler ever reads of a column is rank Geometric(p) +
 * seen-skips from either end (revisit_bpr/modules/neg_samplers.py:90-121), so the split refresh
 * (bpr_adaptive_refresh_begin) sorts only the two ends of every column exactly and BUCKETS the middle
 * (equi-depth bins cut along a coarse histogram of the column, bins in order): 39 us per 20 k-key column
 * instead of 98.  STREAM launches (bpr_train_stream*) read such a snapshot directly — a walk that leaves an
 * exact end finishes inside one bin by taking its <= 64 keys out in order, the same negative as from the
 * fully sorted column, triple for triple — every other reader (bpr_sample_adaptive, bpr_adaptive_pick, the
 * batched STREAM kernel, bpr_adaptive_get_snapshot / _snapshot_ptrs) first has it sorted whole, in place.
 * Columns of 2,048 .. 24,576 items; others — and a column with more than 64 equal-ranked keys in a bin, or an
 * end over 1,024 keys — are sorted whole as before.  Worth +1.6 % on the metric's configuration with the
 * sorter on 32 CUs (the finish costs the launch a wave of occupancy); off by default.
 * *partial_host = 1 while the snapshot the samplers read is a partial one. */
int bpr_adaptive_snapshot_partial(bpr_ctx* ctx, int32_t* partial_host);
/* The refresh SHARDED over the ranks of a multi-GPU job: every rank holds a replica of the item
 * table, so instead of every rank sorting all d columns (an Amdahl term: the sort does not shrink
 * with the number of ranks) rank r sorts columns [f_lo, f_hi) only — _part cuts the keys and
 * sorts those columns into the BACK snapshot —, the caller gathers every rank's columns into the
 * back snapshot of every rank (order [d, I] int32 and sigma [d] fp32: _snapshot_ptrs hands out the
 * device pointers, back != 0 for the back snapshot; an all-gather over RCCL in
 * revisit_bpr/distributed.py) and _publish makes it the snapshot the samplers read.  All in the ctx
 * stream's order.  The reference has no multi-device sampler to mirror. */
int bpr_adaptive_refresh_part(bpr_ctx* ctx, int32_t f_lo, int32_t f_hi);
int bpr_adaptive_refresh_publish(bpr_ctx* ctx);
int bpr_adaptive_snapshot_ptrs(bpr_ctx* ctx, int32_t back, void** order_host, void** sigma_host);
/* ---- multi-GPU inside the library (the reference's DDP launcher, experiments/launcher.py:
 * 35-73, is never enabled by a config, so there is no reference behaviour to mirror) ------------------
 * One RCCL communicator per ctx (librccl.so is opened at run time: no link-time dependency).
 * bpr_comm_unique_id: rank 0 fills BPR_COMM_ID_BYTES bytes of HOST memory (ncclGetUniqueId) and ships
 * them to the other ranks out of band; bpr_comm_init: every rank, collectively (ncclCommInitRank);
 * it also cuts the reconciliation BASE from the item table as it is now (identical on every rank).
 * bpr_item_sync: the steady-state step of the item-table reconciliation — fold the all-reduced
 * deltas of the reconciliation in flight into the live replica (one period late), cut this rank's
 * new delta, all-reduce it on the communicator's own stream under whatever the ctx stream does next
 * (Q <- Q_base + sum_r (Q_r - Q_base); the base is updated from the all-reduced sum only, so it
 * stays bit-identical on every rank).  bpr_item_sync_finish folds the last one in.  With a
 * communicator of world > 1, bpr_adaptive_refresh sorts d / world factors per rank and all-gathers
 * the orders (bpr_adaptive_refresh_part / _publish) when world divides d.
 * revisit_bpr/distributed.py runs the same protocol through torch.distributed (RCCL or gloo). */
#define BPR_COMM_ID_BYTES 128
int bpr_comm_unique_id(void* id_host);
int bpr_comm_init(bpr_ctx* ctx, const void* id_host, int32_t rank, int32_t world);
/* bpr_comm_destroy closes a hot tier still open (folds the exchange in flight and this rank's uncut deltas into the
 * item table) — call it while the tables are alive; bpr_ctx_destroy frees the communicator too but writes NOTHING
 * into the caller's tables (they may be gone by then). */
int bpr_comm_destroy(bpr_ctx* ctx);
int bpr_item_sync(bpr_ctx* ctx);
int bpr_item_sync_finish(bpr_ctx* ctx);
/* The bases follow the tables when they are re-bound (another shape or buffer).  A table overwritten
 * IN PLACE (checkpoint restore, restore-best) is invisible to the library: call this afterwards,
 * on every rank, with identical tables — nothing may be in flight that should still be applied. */
int bpr_item_sync_rebase(bpr_ctx* ctx);
/* Two tiers inside the library (see bpr_hot_exchange below): bpr_comm_hot_tier sets the hot set
 * (the same list on every rank), allocates the exchange buffers and turns the tier on;
 * bpr_hot_sync after every STREAM launch (or sub-launch) folds the hot exchange in flight, cuts the
 * launch's hot deltas and all-reduces them on the communicator's stream; bpr_item_sync stays the
 * per-period step of the cold rows (call it right after bpr_hot_sync); bpr_item_sync_finish folds
 * both.  Every collective of the ctx's communicator runs on the communicator's stream in program
 * order (bpr_adaptive_refresh's all-gather included: with a communicator it IS collective — every
 * rank must call it the same number of times, in the same place of the sequence). */
int bpr_comm_hot_tier(bpr_ctx* ctx, const int32_t* items_host, int32_t H, const uint32_t* counts_host);
int bpr_hot_sync(bpr_ctx* ctx);
/* The side stream of the split refresh (a hipStream_t of the ctx's device; NULL = a plain
 * non-blocking stream created by the library on first use).  The caller keeps ownership. */
int bpr_set_side_stream(bpr_ctx* ctx, void* hip_stream);
/* Streams restricted to a subset of the CUs (hipExtStreamCreateWithCUMask): cu_mask holds
 * mask_words 32-bit words, bit i of the mask = CU i in the driver's numbering (on MI300-class
 * parts bits are dealt round-robin over the 8 XCDs, so a contiguous bit range takes equally from
 * each); mask_words = 0 creates a plain non-blocking stream.  The STREAM kernel is bound by the L2
 * atomic units and leaves most CU cycles idle, so the split refresh's sort runs beside it on a
 * disjoint CU set: create two complementary streams, hand one to bpr_ctx_create / bpr_set_stream
 * and the other to bpr_set_side_stream.  No reference counterpart (the reference has no streams). */
int bpr_stream_create(int device_id, const uint32_t* cu_mask, int32_t mask_words, void** stream_out);
int bpr_stream_destroy(void* hip_stream);
/* AdaptiveSampler.sample: factor ~ |p_uf|·sigma_f, rank ~ Geometric(p) clamped to #unseen,
 * orientation by sign(p_uf), pick the rank-th unseen item of the snapshot order.
 * factor_out / rank_out (int32 [B], nullable) expose the intermediate draws for parity tests;
 * rank_out is the 0-based rank counted from the top, as in neg_samplers.py:96-100. */
int bpr_sample_adaptive(bpr_ctx* ctx, const int32_t* users, int64_t B, float p, uint64_t seed,
                        uint64_t offset, int32_t* neg_out, int32_t* factor_out, int32_t* rank_out);
/* Deterministic half of AdaptiveSampler.sample (neg_samplers.py:109-121): given factor and rank
 * (0-based from the top) return the rank-th unseen item in the snapshot order of that factor. */
int bpr_adaptive_pick(bpr_ctx* ctx, const int32_t* users, const int32_t* factor,
                      const int32_t* rank, int64_t B, int32_t* neg_out);
/* Copy the snapshot to caller buffers (either may be NULL): order [d*I] int32, sigma [d] fp32. */
int bpr_adaptive_get_snapshot(bpr_ctx* ctx, int32_t* order_out, float* sigma_out);

/* ---- the hot path ------------------------------------------------------------------------- */
/* BPR.forward train branch (model.py:48-68): logits_pos/neg [B] (nullable), scalars as above. No
 * parameter is modified.  Used by the eval-free "forward only" callers and by parity tests. */
int bpr_forward(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, const int32_t* neg,
                int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars);

/* STRICT phase A — BPR.forward + loss.backward() (model.py:48-68, trainer.py:76): as bpr_forward,
 * and accumulates the per-row gradients of the batch into the ctx's private accumulators. */
int bpr_forward_grad(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, const int32_t* neg,
                     int64_t B, float* out_logits_pos, float* out_logits_neg, float* out_scalars);
/* STRICT phase B — optimizer.step(); optimizer.zero_grad() (trainer.py:79-81): one optimizer step
 * on every row touched since the last apply, then clears the accumulators. */
int bpr_apply(bpr_ctx* ctx);
/* Drop accumulated gradients without applying them (a forward that was never stepped). */
int bpr_discard_grad(bpr_ctx* ctx);
/* Copy accumulated gradients to dense caller buffers for tests (any may be NULL):
 * gP [U,d], gQ [I,d], gbias [I].  Untouched rows read as zero. */
int bpr_get_grad(bpr_ctx* ctx, float* gP, float* gQ, float* gbias);

/* One reference training iteration (example.py:172-180): sample (if sampler != GIVEN) →
 * forward → backward → optimizer step.  mode STRICT = phases A+B; mode STREAM = one fused launch
 * (SGD only).  `neg` is read when sampler == BPR_NEG_GIVEN, otherwise (if non-NULL) it receives
 * the sampled negatives.  seed/offset as in bpr_sample_uniform; adaptive_p = Geometric p.
 * BPR_NEG_DYNAMIC: mode STREAM only (STRICT: BPR_ERR_UNSUPPORTED — draw with bpr_sample_dynamic, step with
 * BPR_NEG_GIVEN).  BPR_NEG_WARP: mode STREAM only (STRICT: BPR_ERR_UNSUPPORTED); `neg` receives -1 for a skipped
 * triple. */
int bpr_step(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg, int64_t B,
             int32_t mode, int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
             float* out_logits_pos, float* out_logits_neg, float* out_scalars);

/* STRICT epoch driver — `for batch in loader: sample; forward; backward; step` (example.py:172-180,
 * trainer.py:64-83) with the loop on the host side of the library, so that the reference's exact
 * mini-batch semantics (any optimizer) cost three kernel launches per batch and no interpreter
 * time.  users/pos [n] are the epoch's triple stream (already shuffled); batches of B consecutive
 * triples; neg_scratch [>= B] int32 receives each batch's negatives (sampler != GIVEN) or, for
 * BPR_NEG_GIVEN, is the full [n] negative stream.  refresh_every > 0 calls bpr_adaptive_refresh
 * at every refresh_every-th batch exactly where AdaptiveSampler.sample does
 * (neg_samplers.py:75,122-123): after that batch's negatives are drawn and before its optimizer
 * step; the batch counter belongs to the ctx and keeps counting across calls (epochs), as the
 * sampler's _iteration_cnt does (bpr_set_sampler_iter rewinds it).  With lazy optimizers the
 * refresh flushes first.  out_scalars accumulates over the epoch.  BPR_NEG_DYNAMIC, BPR_NEG_WARP:
 * BPR_ERR_UNSUPPORTED, checked before the device is touched. */
int bpr_train_strict(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg_scratch,
                     int64_t n, int64_t B, int32_t sampler, float adaptive_p, uint64_t seed,
                     uint64_t offset, int64_t refresh_every, float* out_scalars);

/* STREAM throughput entry (train_one_epoch's inner loop, example.py:172-180, over n triples in ONE
 * launch): users/pos are the (already shuffled) triple stream resident in HBM.  `max_inflight`
 * bounds how many triples are processed concurrently (0 = fill the chip); see DESIGN.md §staleness.
 * A model's item_bias is read and updated, for the duration of the launch, in a table of the
 * library's own (one item per 128-byte line: DESIGN.md §9.5), filled from the bound vector in stream
 * order before the launch and written back after it: the bound vector is current once the launch
 * has completed on the ctx stream, not while it runs.
 * BPR_NEG_DYNAMIC (plain SGD, as every sampler here): each triple's negative is the hardest of bpr_set_dynamic's M
 * candidates under the user row the kernel holds in registers and the item rows as it reads q_j (hot-row deltas
 * included); `neg`, if non-NULL, receives the picks.  Such a launch never takes the LDS tier (bpr_set_hot_lds).
 * BPR_NEG_WARP (plain SGD): the WARP objective above with bpr_set_warp's (max_sampled, margin), scored as
 * BPR_NEG_DYNAMIC scores; `neg`, if non-NULL, receives the violators, -1 for a skipped triple; out_scalars as stated
 * there.  Never the LDS tier either. */
int bpr_train_stream(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg,
                     int64_t n, int32_t sampler, float adaptive_p, uint64_t seed, uint64_t offset,
                     int64_t max_inflight, float* out_scalars);
/* The same launch, whose epilogue ALSO cuts the keys of the next adaptive snapshot from the item
 * table as the launch leaves it — the first half of bpr_adaptive_refresh_begin, done in the pass
 * that folds the hot rows (one kernel and one kernel boundary less between two launches).  The
 * next bpr_adaptive_refresh_begin then only queues the sort, provided the item table was not
 * touched in between: every ctx call that moves it drops the cut, but writes the library cannot
 * see (bpr_item_fold*, the caller's own kernels) must not happen there.  n must be > 0. */
int bpr_train_stream_cut(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg,
                         int64_t n, int32_t sampler, float adaptive_p, uint64_t seed,
                         uint64_t offset, int64_t max_inflight, float* out_scalars);
/* The same launch with the cut taken OFF the launch stream (r4): the keys of the next snapshot are cut
 * by a read-only pass on the split refresh's side stream, behind this launch and BESIDE the next one —
 * the launch stream runs launch after launch with nothing in between.  Two consequences, both inside
 * the asynchrony the STREAM mode already has: the snapshot's point in time is "after
 * this launch, plus whatever the next launch did in the ~20 us the cut takes"; and the hot rows'
 * deltas are NOT folded into the item table by the launch — every other entry point of the ctx folds
 * them first (the table is whole for whoever looks through the library), and a caller who reads the
 * item table's storage directly (eval, checkpoint) calls bpr_hot_fold before.  out_scalars is added
 * to by the side-stream pass: read it after bpr_hot_fold or a device synchronisation.
 * r6 (default; bpr_set_tuning "acut_fold" 0 restores the form above): only the TRANSPOSE of the keys leaves the launch
 * stream — the fold of the hot block, the loss sums and the item_bias write-back stay on it (k_stream_epilogue, a few
 * microseconds) — so the item table is whole after every launch (bpr_hot_fold is a no-op), out_scalars arrives on the
 * launch stream, and the LDS tier (bpr_set_hot_lds) stays in use.
 * BPR_NEG_DYNAMIC and BPR_NEG_WARP have no snapshot to cut: BPR_ERR_UNSUPPORTED. */
int bpr_train_stream_acut(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg,
                          int64_t n, int32_t sampler, float adaptive_p, uint64_t seed,
                          uint64_t offset, int64_t max_inflight, float* out_scalars);
int bpr_hot_fold(bpr_ctx* ctx);

/* BATCHED STREAM — the single-launch throughput path for every optimizer kind (SGD, momentum /
 * Nesterov, Adam, RMSprop, Adagrad; configs/RQ3/time-split/ada-sampling-adam.yaml.j2:169-175 and 14 of the
 * 22 BPR configs step torch.optim.Adam at experiments/trainer.py:79-81).  users/pos [n] are the
 * shuffled triple stream (bpr_shuffle_epoch; NOT grouped by user); triple k belongs to virtual
 * mini-batch k / B, i.e. optimizer step (steps so far) + 1 + k / B.  Per row the gradients of one
 * virtual batch are summed and applied as ONE torch.optim step (dense semantics: untouched rows
 * catch up lazily), every gradient being evaluated on the rows as of the previous step.  Executed
 * by one group (max_inflight = 1) this IS the reference's mini-batch loop; with the chip full,
 * triples of up to max_inflight (0 = fill the chip) consecutive stream positions run concurrently
 * and see rows that may be a few steps stale.  Advances the step counter by
 * ceil(n / B); bpr_flush_lazy / bpr_adaptive_refresh bring rows to "now" (call bpr_flush_lazy
 * before reading the tables: eval, checkpoint, item all-reduce).  sampler / seed / offset / neg /
 * out_scalars as bpr_train_stream.
 * r4: for 16 <= B <= 2048 the launch first marks the triples whose user occurs once in its virtual
 * batch; such a user row takes its optimizer step at once, under the row's lock, instead of parking
 * the gradient for the row's next visitor (same arithmetic, bit-identical in the max_inflight = 1
 * limit).  On by default except for Adam on a model with item_bias;
 * bpr_set_tuning(ctx, "vs_direct", 0 / 1) forces it off / on (a measurement and test aid).
 * BPR_NEG_DYNAMIC, BPR_NEG_WARP: BPR_ERR_UNSUPPORTED, checked before the device is touched
 * (bpr_train_stream_batched_scored, below, is this launch with them). */
int bpr_train_stream_batched(bpr_ctx* ctx, const int32_t* users, const int32_t* pos, int32_t* neg,
                             int64_t n, int64_t B, int32_t sampler, float adaptive_p,
                             uint64_t seed, uint64_t offset, int64_t max_inflight,
                             float* out_scalars);
/* BATCHED STREAM with the scored samplers: bpr_train_stream_batched's launch — the same virtual mini-batches, one
 * torch.optim step per row and batch under any optimizer kind, the same max_inflight, vs_direct and step counter —
 * with sampler = BPR_NEG_DYNAMIC or BPR_NEG_WARP (any other kind: BPR_ERR_INVALID).  The draw is the one stated at
 * bpr_sample_dynamic and bpr_sample_warp above, with the ctx's bpr_set_dynamic / bpr_set_warp values, for counter
 * offset + k of triple k (the uniform sampler's candidate stream, item weights, the rank fallback, duplicates kept;
 * the pick rules and NaN rules as stated there).  Two rules are this entry point's own:
 *   views      every row the draw reads — p_u, q_i and each candidate's item row and bias — is the row AS OF STEP
 *              t - 1 of the triple's virtual batch t (its pending step applied, the zero-gradient steps since
 *              replayed), as every gradient of the batch is; nothing is written by the draw.  On rows that do not
 *              move the picks and tries are bpr_sample_dynamic's and bpr_sample_warp's bit for bit (the same
 *              reduction at every width); with max_inflight = 1 that holds for the launch's first virtual batch on
 *              flushed tables, and later batches draw on the tables the earlier batches left.
 *   skipped    a BPR_NEG_WARP triple without a violator contributes to no row (it parks no gradient, closes no step,
 *              takes no lock) and to no scalar, yet it belongs to virtual batch k / B: the launch advances the step
 *              counter by ceil(n / B) whatever was skipped, and a row touched by skipped triples only is an
 *              untouched row — it catches up lazily with zero gradient, as a dense torch.optim step does.
 * The step: BPR_NEG_DYNAMIC as bpr_train_stream_batched's on the pick; BPR_NEG_WARP with L = log(max(1,
 * floor(n_unseen / tries))) in the place of sigma(-x) in the three rows' gradients and the bias gradients, the L2
 * terms as they are.  neg [n] or NULL receives the picks (-1: skipped); tries [n] or NULL receives BPR_NEG_WARP's
 * tries (0: skipped) and 1 for every BPR_NEG_DYNAMIC triple.  out_scalars (+=): BPR_NEG_DYNAMIC as
 * bpr_train_stream_batched; BPR_NEG_WARP as bpr_train_stream's, over the stepped triples: sum L (margin - x_i + x_k),
 * the L2 term, sum |x_i - x_k|, the stepped count.  No seen CSR, users or pos NULL, B < 1, unapplied STRICT
 * gradients: BPR_ERR_INVALID, nothing launched.  STRICT (bpr_train_strict, bpr_step) keeps refusing both kinds. */
int bpr_train_stream_batched_scored(bpr_ctx* ctx, const int32_t* users, const int32_t* pos,
                                    int32_t* neg /* or NULL */, int32_t* tries /* or NULL */, int64_t n, int64_t B,
                                    int32_t sampler, uint64_t seed, uint64_t offset, int64_t max_inflight,
                                    float* out_scalars);
/* DataLoader(shuffle=True, generator=manual_seed(seed)) stand-in (example.py:307-321,
 * experiments/bpr/exp.py:109-118) without the by-user grouping of bpr_plan_epoch: a seeded
 * pseudo-random permutation of the n training triples, computed on device.  Outputs must not alias
 * the inputs. */
int bpr_shuffle_epoch(bpr_ctx* ctx, const int32_t* users_in, const int32_t* pos_in, int64_t n,
                      uint64_t seed, int32_t* users_out, int32_t* pos_out);

/* ONE chunk of that plan without planning the epoch: the triples of chunk `index` (the same member
 * set bpr_plan_epoch(seed) puts there, grouped by user; the order of a user's triples may differ),
 * found through the INVERSE of the permutation — pi^-1 of [index * chunk, (index + 1) * chunk) — and
 * sorted by user: ~200 k keys instead of the whole epoch.  users_out / pos_out [min(chunk, n - index *
 * chunk)].  The plan does not depend on the model: with on_side != 0 it is queued on the split
 * refresh's side stream behind the sort in flight (bpr_adaptive_refresh_begin must have been
 * called), and bpr_adaptive_refresh_commit then waits for both — the chunk after next is planned in
 * the time the sorter idles, nothing is planned on the launch stream (fast.StreamTrainer(jit_plan)). */
int bpr_plan_chunk(bpr_ctx* ctx, const int32_t* users_in, const int32_t* pos_in, int64_t n, int64_t chunk,
                   uint64_t seed, int64_t index, int32_t* users_out, int32_t* pos_out, int32_t on_side);

/* STREAM options.  grouped_by_user = 1 promises that inside every chunk handed to
 * bpr_train_stream the triples of a user are contiguous (the output of bpr_plan_epoch): a user
 * whose triples all fall in one run of `run_len` consecutive triples is then owned by one
 * wavefront group for the whole launch and its row is written back with a plain store; with 0
 * (default) every user-row update is an atomic add.  run_len = consecutive triples one
 * group walks with the user row held in registers: 1..30, or 0 (default) = chosen per launch —
 * 8 when runs of 8 fill the launch stream's CUs more than once; for smaller launches the shortest
 * runs of 4..8 triples that fit those CUs in one residency, one run per group (a small launch
 * ends when its slowest group does; with max_inflight > 0 the bound is min(those CUs' capacity,
 * max_inflight) groups).  bpr_stream_run_len: what the last STREAM launch used. */
int bpr_set_stream_opts(bpr_ctx* ctx, int32_t grouped_by_user, int32_t run_len);
int bpr_stream_run_len(bpr_ctx* ctx);

/* Hot item rows.  On popularity-skewed data the STREAM kernel is limited by fp32 atomics queueing
 * on the memory channels that happen to hold the most popular item rows (rows are scattered over
 * the table, the load per channel is uneven).  bpr_plan_epoch therefore counts the training
 * positives per item (once per training set) and the `hot_rows` most popular rows (default 256)
 * take their STREAM updates in a compact block of delta rows — each placed in the slot whose
 * channels are least loaded, counting what the rows left in Q put on every channel, so that the
 * whole launch is spread evenly; optionally `replicas` (1, 2, 4 or 8; default 1) of the block, a
 * wavefront adds to one, every reader adds them all to the base row — folded into Q right after
 * every STREAM launch.  Same algebra
 * as updating Q directly, up to the association of fp32 sums.  hot_rows = 0 turns it off.  Takes
 * effect at the next bpr_plan_epoch. */
int bpr_set_hot_rows(bpr_ctx* ctx, int32_t hot_rows, int32_t replicas);
/* The LDS tier of the hot block (r6).  Once the adaptive sampler has a trained model to adapt to, its
 * negatives concentrate on the head of the dominant factors' orders (neg_samplers.py:84-121) — 40-60 % of
 * them, and half of the positives, fall on a few hundred item rows, ~800 updates per row and launch, each one
 * four memory-side line requests plus the read of a delta row those requests keep dropping from the L2s.
 * With rows > 0, STREAM launches that fill the chip at least twice run ONE workgroup per CU (up to 1,024
 * threads, persistent over its share of the runs) that keeps a private fp32 delta block for the `rows` most
 * popular hot rows in LDS beside its groups' seen bitmaps (as many as fit the CU's 160 KiB; d = 128, ML-20M:
 * 128 rows): an update of such a row is an LDS add, its value is Q + the workgroup's own LDS delta, and the
 * rows a workgroup touched are added to the global delta block at its exit (so the fold, the cut, the hot tier
 * of several GPUs and the exact-sum property are what they were).  SEMANTICS: a workgroup sees the other
 * workgroups' updates of these rows one launch late — the staleness `learning rate x triples per launch`
 * that the multi-GPU budget prices (revisit_bpr/fast.py lag_within_budget: inside at the
 * reference's lr 0.001 and 0.01, outside at 0.05), which is why it is off by default and the trainers switch
 * it on by that rule.  With max_inflight = 1 (one group) it is exactly sequential SGD.  always = 1: also for
 * launches that do not fill the chip (tests).  Needs a hot block (bpr_plan_epoch / bpr_set_hot_items), d in
 * {32, 64, 128, 256, 512, 1024}, a snapshot sorted whole (the groups' seen structure is the LDS bitmap, or the staged
 * sorted list when the bitmaps would not leave 32 KB for rows: item tables past ~60 k items); otherwise the plain
 * kernel runs.  Under the hot tier (bpr_hot_tier_begin) only the first launch after a bpr_hot_exchange with cut = 1
 * (or a bpr_sync_cut) takes it: a later one, whose block still holds the earlier launches' deltas, runs the plain kernel.
 * bpr_stream_lds_rows: LDS rows of the last STREAM launch (0 = the plain kernel ran). */
int bpr_set_hot_lds(bpr_ctx* ctx, int32_t rows, int32_t always);
int bpr_stream_lds_rows(bpr_ctx* ctx);
/* Test and measurement aids, per ctx (nothing in the library reads the environment per launch):
 *   "seen"      0 = by shape (default), 1 = binary search in the CSR, 2 = LDS bitmap, 3 = staged list —
 *               the structure the sampling kernels answer "has u seen c?" from;
 *   "vs_direct" -1 = by optimizer (default), 0 / 1 = lonely user rows of the batched STREAM kernel step
 *               through the gradient buffer / directly under the row's lock;
 *   "adam_closed" 1 (default) / 0 = Adam's missed zero-gradient steps replayed in closed form / by the loop;
 *   "refresh_sub" 0 = by shape (default), 1 | 2 | 4 = workgroups per column of the in-LDS snapshot sort;
 *   "partial_snapshot" 0 / 1, "partial_target" 1..1024: bpr_adaptive_snapshot_partial above;
 *   "binned_sort" 1 (default) / 0: tables of 2,048 .. 20,480 items have their snapshot columns ordered by
 *               k_sort_binned (equi-depth bins + ranking inside the bin: the same stable descending order as
 *               the radix sort, bit for bit, in ~0.4 of its time; up to 131,071 items with several workgroups per
 *               column, k_sort_binned_split and, from 65,536 items on, its 17-bit-id form) / by the radix sort (a
 *               test and measurement aid);
 *   "binned_split" 0 (default: workgroups per column by table size) / 1..16 (tests and measurements force the split
 *               kernel: on small tables, or with more workgroups than the table needs; a value too small for the
 *               table is raised until a stretch fits a workgroup);
 *   "lds_block" 0 (default: 1,024 threads for d <= 256 at 32-lane groups, 512 above) / a multiple of 64: threads per
 *               workgroup of the LDS-tier kernel (bpr_set_hot_lds) — fewer groups leave more LDS for hot rows;
 *   "plan_input_sorted" 0 (default) / 1: a PROMISE that the users_in handed to bpr_plan_epoch are sorted by user id (the
 *               triple list in CSR order, as every loader of this repository makes it): the plan — same output — then
 *               takes one radix pass over the chunk bits instead of three over (chunk, user);
 *   "acut_fold" 1 (default, r6) / 0: bpr_train_stream_acut keeps the fold of the hot block (+ loss sums, bias write-back)
 *               on the launch stream and sends only the transpose of the snapshot's keys to the side stream / r4's form
 *               (nothing folded until bpr_hot_fold: the LDS tier is then not used);
 *   "lds_tail"  0..50 (default 12): percent of a launch's triples the LDS-tier kernel deals in runs of run_len / 2 and
 *               run_len / 4 at the end of every persistent workgroup's share (a workgroup is over when its last run is). */
int bpr_set_tuning(bpr_ctx* ctx, const char* key, int32_t value);
/* The item_bias during STREAM launches (models/bpr/model.py:101-110; the RQ configs switch it on).
 * k_stream works on a table of its own with ONE item per 128-B line (in the dense vector 32 items share a
 * line and every bias load queues behind their adds at the memory side); each launch fills it from the
 * caller's vector and its epilogue writes it back.  bpr_set_bias_tracking(ctx, 1): the fill is skipped
 * while the table is known to equal the vector — written back by the previous launch, no entry point of
 * the library has written the vector since — which leaves writes the library cannot see: after any
 * write of the caller's own to item_bias (optimizer step on the tensor, checkpoint load, zero_()) call
 * bpr_bias_written before the next launch.  Off by default (every launch refills). */
int bpr_set_bias_tracking(bpr_ctx* ctx, int32_t on);
int bpr_bias_written(bpr_ctx* ctx);
/* Heavy users (more seen items than `threshold`, default 256; -1 = none) get an I-bit seen bitmap in
 * HBM, built synchronously by the first sampling STREAM launch after the seen CSR was bound; the
 * bitmaps take at most `max_bytes` (default 1 GiB; 0 keeps the current cap) — the threshold is
 * doubled until they fit. */
int bpr_set_heavy_users(bpr_ctx* ctx, int32_t threshold, int64_t max_bytes);
/* The heavy table as the last sampling STREAM launch used it: `n` = users with a bitmap row (0: no table, or
 * not built yet), `threshold` = the threshold it ended at (the requested one, doubled until the rows fit). */
int bpr_heavy_users(bpr_ctx* ctx, int64_t* n, int32_t* threshold);

/* ---- two-tier item reconciliation, HOT tier (several GPUs; no reference counterpart — the
 * reference's latent DDP, experiments/launcher.py:35-73, would all-reduce every gradient of every
 * step).  At full-size launches per rank, N replicas each pour a whole launch into the same few
 * popular rows before anybody sees the others' updates; those rows — and only those — are therefore
 * exchanged after EVERY launch (or sub-launch) as a block of H x d floats (128 KB at H = 256,
 * d = 128), while the cold rows keep the per-period all-reduce of bpr_item_fold_delta.
 *
 * bpr_set_hot_items  the hot set as the caller gives it — the ranks must agree on it (the H most
 *                    popular items of the WHOLE training set); items_host [H] distinct item rows in
 *                    the canonical order of the exchange buffers, counts_host [I] (or NULL) only
 *                    steers the slot placement.  H = 0 returns to bpr_set_hot_rows' own choice.
 * bpr_hot_tier_begin hot_base [H, d] <- the hot rows of the item table (replicas identical at this
 *                    point); from here on STREAM launches leave their hot-row deltas in the block.
 * bpr_hot_exchange   one pass over the block on the ctx stream:
 *                      fold_prev: hot_base += tot   (tot = all-reduced sum of the previous exchange)
 *                      cut:       tot <- this rank's deltas of the launches since, deltas <- 0
 *                      Q[hot rows] <- hot_base + tot;  cold_base (optional, [I, d]): same rows <- same
 *                    The caller all-reduces `tot` (SUM) between two calls.  hot_base only ever takes
 *                    all-reduced sums: it stays bit-identical on every rank.  cold_base keeps the
 *                    cold tier's delta of a hot row at exactly zero.
 * bpr_hot_tier_end   launches fold their hot block themselves again (call bpr_hot_exchange with
 *                    fold_prev as due and cut = 1 first, all-reduce, then once more with cut = 0). */
int bpr_set_hot_items(bpr_ctx* ctx, const int32_t* items_host, int32_t H, const uint32_t* counts_host);
int bpr_hot_rows(bpr_ctx* ctx, int32_t* rows_host);
int bpr_hot_tier_begin(bpr_ctx* ctx, float* hot_base);
int bpr_hot_exchange(bpr_ctx* ctx, float* hot_base, float* tot, int32_t fold_prev, int32_t cut,
                     float* cold_base);
int bpr_hot_tier_end(bpr_ctx* ctx);
/* Everything a rank does to the item table between two launches, in ONE pass (r4): the hot-tier
 * exchange step (as bpr_hot_exchange with cut = 1), the cold tier's step (cold_mode 2: as
 * bpr_item_fold_delta; 1: as bpr_item_delta; 0: none) and the cut of the next adaptive snapshot's
 * keys (as bpr_train_stream_cut's epilogue: the next bpr_adaptive_refresh_begin only queues the
 * sort).  Call it right after a bpr_train_stream_cut issued under the hot tier — that launch leaves
 * its epilogue (the loss partials) to this pass — and all-reduce hot_tot and cold_tot afterwards.
 * Four kernels and their boundaries (53 us measured) become one. */
int bpr_sync_cut(bpr_ctx* ctx, float* hot_base, float* hot_tot, int32_t hot_fold_prev, float* cold_base,
                 float* cold_own, float* cold_tot, float scale, int32_t cold_mode);

/* Epoch order for STREAM mode — replaces DataLoader(shuffle=True, generator=manual_seed(seed))
 * (example.py:307-321; experiments/bpr/exp.py:109-118): a seeded pseudo-random partition of the n
 * training triples into ceil(n/chunk) chunks of `chunk` triples (the last may be shorter); inside a
 * chunk triples are grouped by user.  users_out/pos_out [n] must not alias the inputs. */
int bpr_plan_epoch(bpr_ctx* ctx, const int32_t* users_in, const int32_t* pos_in, int64_t n,
                   int64_t chunk, uint64_t seed, int32_t* users_out, int32_t* pos_out);

/* Dense-optimizer equivalence: torch's dense Adam / momentum move EVERY row on every
 * step.  The strict path replays the missed zero-gradient steps lazily when a row is next
 * touched; this brings all rows to the current step (call before eval / checkpoint / all-reduce). */
int bpr_flush_lazy(bpr_ctx* ctx);
/* The same for the item table (and item_bias) only: what the item reconciliation across GPUs and
 * the sampler snapshot need — the user shard of a rank is read by nobody else and stays lazy. */
int bpr_flush_items(bpr_ctx* ctx);
/* Global optimizer step counter t (number of bpr_apply calls); settable for checkpoint resume. */
int bpr_get_step_host(bpr_ctx* ctx, int64_t* step_host);
int bpr_set_step(bpr_ctx* ctx, int64_t step);
/* AdaptiveSampler._iteration_cnt of the bpr_train_strict loop (neg_samplers.py:75): batches drawn so
 * far; 0 at ctx creation.  Settable so a resumed run refreshes at the same iterations. */
int bpr_set_sampler_iter(bpr_ctx* ctx, int64_t iteration);

/* ---- evaluation (E3): ROC-AUC of a block of score rows — the quantity of the reference's RocAucMany /
 * RocAucManySlow (revisit_bpr/metrics/auc.py:70-130: every (positive, negative) pair of a row; 1 of the 14 metrics of
 * its ML-20M / MSD configs) without the [B, I, I] comparison or a sort per row: scores [n, I] fp32 row-major (masked
 * entries carry their mask value and count as negatives, as in the reference's eval loop), positives of row r =
 * pos_items[pos_indptr[r] .. pos_indptr[r + 1]) (pos_indptr [n + 1] int64, need not start at 0).
 * THE CONTRACT, for one row with scores s[0 .. I) and the set Pos of its listed ids:
 *   wins = #{(p, n) : p in Pos, n not in Pos, s[p] > s[n]} with IEEE '>': false whenever either side is NaN (a NaN
 *          positive wins nothing, a NaN negative is beaten by nothing and still counts in I - T), -0 == +0,
 *          subnormals compare by value, +-inf are ordinary values;
 *   T = |Pos|;  auc_out[r] = (float)((double)wins / ((double)T * (double)(I - T)));
 *   NaN when T == 0 or T == I (0 / 0, as the metric classes) and when T > 4,096 ("not computed": the caller's
 *   sort-based path takes the row).  The result is a function of the row alone, not of the order of its ids.
 * PRECONDITIONS, which the kernel cannot check without a fault path: every id lies in [0, I) (another id reads out of
 * bounds), and the ids of a row are unique (a repeated id would count as two positives and win twice;
 * evaluation.evaluate_topk removes repeats before the call).
 * Held bit for bit to an all-pairs count by tests/test_gpu_auc.py (tests/auc_model.py).  Context-free: runs on
 * `hip_stream`. */
int bpr_auc_rows(const float* scores, int64_t n, int64_t I, const int64_t* pos_indptr, const int32_t* pos_items,
                 float* auc_out, void* hip_stream);

/* ---- recommendation: the k best unseen items of a list of users (the reference ranks through full logits:
 * example.py:195-230, the preds.jsonl / user-metrics.jsonl savers of experiments/options.py:319-351).  One fused
 * kernel (csrc/bpr_topk.hip): s(u, i) = <P[u], Q[i]> (+ item_bias[i]) in fp32 over all I items, item 0 and the
 * items of the user's seen row (the CSR of bpr_bind_seen_csr: int64 [U+1], int32 sorted per row; NULL = only item 0)
 * left out, and no [n, I] buffer anywhere.  items_out / scores_out [n, k]: rows sorted by score descending, ties by
 * ascending item id; a row with fewer than k eligible items ends in item -1 / score -inf.  A NaN score (a NaN in a
 * row, 0 * inf, inf - inf) is never returned, so such a row may end in padding although items are left; +inf and -inf
 * scores are ordered like any other, and a real item scoring -inf keeps its id (tests/test_gpu_chain.py holds all of
 * this, and the score's bits, to tests/chain_model.py).  The result is a pure
 * function of the inputs: its bits do not depend on n, on a user's place in the list (which may repeat users) or on
 * item_slices (0 = the library chooses; s > 1 cuts the item range over s workgroups per user tile, for lists too
 * short to fill the chip, and needs the workspace).  d in [1, 1024], 1 <= k <= 128 (more: BPR_ERR_INVALID),
 * item_slices in [0, 64], n < 2^31.  User ids are not checked.  Arguments are validated before the device is touched; n == 0
 * is BPR_OK.  Context-free: runs on `hip_stream` of the current device. */
/* bytes of device workspace bpr_topk_rows needs for this shape (0 with one slice; with s slices s * n * k * 8;
 * item_slices 0: never less than for a smaller n) */
int bpr_topk_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int64_t* bytes_host);
/* the slice count a call of this shape runs with (item_slices 0: the library's choice; a given count is capped at
 * the item tiles).  Passing it back as item_slices makes bpr_topk_workspace answer exactly that call's need — 0
 * for one slice — instead of the never-shrinking bound of item_slices 0. */
int bpr_topk_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int32_t* slices_host);
int bpr_topk_rows(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                  const int32_t* users, int64_t n,
                  const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                  int32_t k, int32_t item_slices /* 0 = choose */,
                  void* workspace, int64_t workspace_bytes,
                  int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);

/* ---- the item filter of the whole-catalogue calls: "only these items" (in stock, of a category, licensed, not on a
 * block list) as one more eligibility rule inside the kernel, beside "not item 0" and "not in the seen row".
 * item_filter is a device bitmap of uint32 words, bit (i & 31) of word (i >> 5) set = item i is eligible;
 * 4 * ceil(I / 128) words long (a whole number of the kernels' item tiles), its start 16-byte aligned (else
 * BPR_ERR_INVALID under the _filtered entry's name), bits at or past I zero (and never read as items if they are not).
 * Item 0 stays out whatever its bit says; the seen CSR and the NaN rule apply as before.  csrc/bpr_item_filter.h
 * states the layout for host and device.  NULL: the call IS its unfiltered parent — the same kernel instantiation,
 * the same bits.  Each _filtered entry has its parent's signature with item_filter behind seen_indices, its parent's
 * refusals in its parent's order under its own name, and its parent's _workspace / _slices queries (the plan does not
 * look at the filter).
 * Scores are untouched: a filtered result is, bit for bit, the unfiltered ranking restricted to the eligible items,
 * cut to k and padded with -1 / -inf — whatever n, the rows' order, item_slices, and however many tiles held no
 * eligible item and were skipped (a narrow filter costs in proportion to the tiles it touches).
 * bpr_sample_rows_filtered: the k draws are over the eligible items, and log_z_out is the normaliser over the
 * eligible, unseen, non-NaN items only (-inf when there is none), under bpr_sample_rows' tolerance contract. */
int bpr_topk_rows_filtered(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                           const int32_t* users, int64_t n,
                           const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                           const uint32_t* item_filter /* [4 * ceil(I / 128)] or NULL */,
                           int32_t k, int32_t item_slices /* 0 = choose */,
                           void* workspace, int64_t workspace_bytes,
                           int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);

/* ---- deep retrieval: bpr_topk_rows for 1 <= k <= 1024, the first stage of a two-stage recommender (candidates for
 * bpr_rerank_rows, a downstream ranker or a business-rule filter).  Its own fused kernel (csrc/bpr_retrieve.hip):
 * the rows' candidate buffers live in the device workspace and are compacted by a sort in LDS, and a bounded number
 * of persistent workgroups walks the user tiles, so the workspace does not grow with n beyond the slices' partial
 * results.  Semantics are bpr_topk_rows' word for word: s(u, i) is the same fp32 fmaf chain plus one bias add (the
 * same bits), item 0 and the user's seen row are left out, rows are sorted by score descending, ties by ascending
 * id, a short row ends in item -1 / score -inf, a NaN score is never returned (the row may then end in padding), +-inf
 * scores are ordered like any other, a real item scoring -inf keeps its id, and the result is a pure function of the
 * inputs (not of n, of a row's place in the list, of repeated users, of item_slices).  For k <= 128 it returns what
 * bpr_topk_rows returns, bit for bit.  d in [1, 1024], item_slices in [0, 64] (0 = the library chooses; a count
 * above 8192 / k or above the item tiles is reduced, not refused: bpr_retrieve_slices reports the count that runs),
 * n < 2^31.  The workspace (8-byte aligned) is needed whenever n > 0.  User ids are not checked.  Arguments are
 * validated before the device is touched; n == 0 is BPR_OK.  Context-free: runs on `hip_stream` of the current
 * device. */
/* bytes of device workspace bpr_retrieve_rows needs for this shape: the persistent workgroups' candidate blocks
 * (constant in n once n passes their reach) plus, with s > 1 slices, s * n * k * 8 of partial results; item_slices
 * 0: never less than for a smaller n */
int bpr_retrieve_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int64_t* bytes_host);
/* the slice count a call of this shape runs with; passing it back as item_slices makes bpr_retrieve_workspace
 * answer exactly that call's need */
int bpr_retrieve_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int32_t* slices_host);
int bpr_retrieve_rows(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                      const int32_t* users, int64_t n,
                      const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                      int32_t k, int32_t item_slices /* 0 = choose */,
                      void* workspace, int64_t workspace_bytes,
                      int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);
/* bpr_retrieve_rows over the eligible items of an item filter (see bpr_topk_rows_filtered) */
int bpr_retrieve_rows_filtered(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I,
                               int32_t d, const int32_t* users, int64_t n,
                               const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                               const uint32_t* item_filter /* [4 * ceil(I / 128)] or NULL */,
                               int32_t k, int32_t item_slices /* 0 = choose */,
                               void* workspace, int64_t workspace_bytes,
                               int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);

/* ---- sampling: k unseen items per user drawn WITHOUT replacement from softmax(s(u, .) / temperature) over the
 * user's eligible items (the Plackett-Luce model) — exploration, and logs that off-policy evaluation can use.  The
 * reference's sampler goes through the [n, I] score matrix and a multinomial; here one fused kernel
 * (csrc/bpr_sample.hip) with bpr_topk_rows' tiling, selection and slices, by the Gumbel-top-k identity: the k largest
 * keys, in descending order, are the k draws in the order drawn.
 * Eligibility and scores are bpr_topk_rows': item 0 and the user's seen row are out; s(u, i) is the same fp32 fmaf
 * chain plus one bias add, the same bits.
 * The draw (csrc/bpr_sample_shared.h; tests/sample_model.py states it in numpy).  Row r has the 64-bit id
 * draw_ids[r] (NULL: the user id).  Item i's 32 random bits are word i & 3 of philox4x32_10 with counter
 * (i >> 2, lo32(draw_id), hi32(draw_id), 3) and key (lo32(seed), hi32(seed)); u = ((bits >> 9) + 0.5f) * 2^-23, exact
 * in fp32 and strictly inside (0, 1); g = -log(-log(u)) with the header's logarithm, a fixed sequence of fp32
 * operations (within 5.34e-7 of float64 for every u); key = fmaf(s, inv_temp, g), inv_temp = 1.0f / temperature in
 * fp32.  Items and keys are therefore a pure function of (tables, user, draw_id, seed, temperature): not of n, of a
 * row's place in the list, of item_slices.  The same user twice with one draw_id is the same row twice; give rows
 * distinct draw_ids (a request counter) for independent draws.
 * items_out [n, k]: the draws in order (key descending, ties by ascending id); scores_out [n, k]: their unperturbed
 * scores s(u, i), bpr_rerank_rows' cand_scores bits; keys_out [n, k] or NULL.  A row with fewer than k eligible
 * items ends in item -1 / score -inf / key -inf.  A NaN score gives a NaN key and is never returned; a +-inf score
 * gives a +-inf key, ordered like any other (+inf is drawn first).
 * log_z_out [n] or NULL: log sum_i exp(s(u, i) * inv_temp) over the row's eligible items whose score is not NaN, the
 * normaliser a propensity needs; -inf for a row with nothing eligible, +inf with an eligible +inf score.  Accumulated
 * online in fp32 with the fast exp / log: held to a tolerance, not to bits, and its bits may depend on item_slices
 * (the slices' sums are combined in slice order); for a fixed slice count they depend on nothing else.
 * d in [1, 1024], 1 <= k <= 128, temperature finite and > 0 with 1.0f / temperature finite (else BPR_ERR_INVALID),
 * item_slices in [0, 64], n < 2^31.  The workspace is 8-byte aligned.  User ids are not checked.  Arguments are
 * validated before the device is touched; n == 0 is BPR_OK.  Context-free: runs on `hip_stream` of the current
 * device. */
/* bytes of device workspace bpr_sample_rows needs for this shape: bpr_topk_workspace's partial results, plus
 * 8 bytes per row and slice (with one slice too) when log_z is wanted; item_slices 0: never less than for a
 * smaller n */
int bpr_sample_workspace(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int32_t want_log_z,
                         int64_t* bytes_host);
/* the slice count a call of this shape runs with (as bpr_topk_slices) */
int bpr_sample_slices(int64_t n, int64_t I, int32_t d, int32_t k, int32_t item_slices, int32_t* slices_host);
int bpr_sample_rows(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                    const int32_t* users, int64_t n, const int64_t* draw_ids /* [n] or NULL = the user id */,
                    const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                    int32_t k, float temperature, uint64_t seed, int32_t item_slices /* 0 = choose */,
                    void* workspace, int64_t workspace_bytes,
                    int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, float* keys_out /* [n,k] or NULL */,
                    float* log_z_out /* [n] or NULL */, void* hip_stream);
/* bpr_sample_rows over the eligible items of an item filter (see bpr_topk_rows_filtered) */
int bpr_sample_rows_filtered(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I,
                             int32_t d, const int32_t* users, int64_t n,
                             const int64_t* draw_ids /* [n] or NULL = the user id */,
                             const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                             const uint32_t* item_filter /* [4 * ceil(I / 128)] or NULL */,
                             int32_t k, float temperature, uint64_t seed, int32_t item_slices /* 0 = choose */,
                             void* workspace, int64_t workspace_bytes,
                             int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */,
                             float* keys_out /* [n,k] or NULL */, float* log_z_out /* [n] or NULL */,
                             void* hip_stream);

/* ---- ranking of held-out items: where each target of a row stands among the user's eligible items (the reference
 * measures through full logits: example.py:195-230 and experiments/bpr/exp.py:369-374, an argsort of I scores per
 * metric object; metrics/auc.py:70-130; metrics/map.py; the user-metrics.jsonl saver of experiments/options.py:319-351).
 * Fused kernels (csrc/bpr_rank.hip), no [n, I] buffer anywhere.  A row r is a user users[r] with the targets
 * tgt_items[tgt_indptr[r] .. tgt_indptr[r + 1]) (tgt_indptr [n+1] int64, need not start at 0; the same user may
 * appear in several rows; at most 112 targets in a row, more: BPR_ERR_INVALID, the caller splits the row).  Item j is
 * ELIGIBLE for row r if 1 <= j < I and j is not in the seen row of users[r] (the CSR of bpr_bind_seen_csr: int64
 * [U+1], int32 sorted and unique per row; NULL = only item 0 is left out): bpr_topk_rows' rule.  s(u, j) =
 * <P[u], Q[j]> (+ item_bias[j]) in fp32, bit for bit the score bpr_topk_rows gives the pair.  For the target t at
 * position p of tgt_items, over the eligible items j != t of its row's user:
 *     rank_out[p]       #{ s_j > s_t, or s_j == s_t and j < t }   (t's index in bpr_topk_rows' order)
 *     not_below_out[p]  #{ s_j >= s_t }                           (not_below - rank = ties that come after t)
 *     score_out[p]      s_t
 * A target that is itself not eligible (id 0, outside [0, I), or seen by the user): rank = not_below = -1, score =
 * -inf; it never faults.  A NaN score is never "before" or ">=" anything.  Other targets of the row count as ordinary
 * eligible items; a duplicated target gets the same answer at both positions.  The result is a pure function of these
 * definitions: it does not depend on n, on the order of the rows, on how a user's targets are spread over rows, or on
 * item_slices (0 = the library chooses; s > 1 cuts the item range over s workgroups per row tile and needs the
 * workspace).  d in [1, 1024], item_slices in [0, 64], n below 2^31 / 112.  User ids are not checked.  Arguments are
 * validated before the device is touched; n == 0 is BPR_OK.  tgt_indptr is read by the kernels, except for ONE host
 * read: the call copies back its two ends and its longest row and waits for `hip_stream` to do so (the launches
 * themselves are asynchronous; the call cannot be captured into a graph).  Context-free: runs on `hip_stream` of the
 * current device. */
/* bytes of device workspace bpr_rank_rows needs for this shape (0 with one slice; with more n * 112 * 12;
 * item_slices 0: never less than for a smaller n) */
int bpr_rank_workspace(int64_t n, int64_t I, int32_t d, int32_t item_slices, int64_t* bytes_host);
/* the slice count a call of this shape runs with (as bpr_topk_slices) */
int bpr_rank_slices(int64_t n, int64_t I, int32_t d, int32_t item_slices, int32_t* slices_host);
int bpr_rank_rows(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                  const int32_t* users, int64_t n,
                  const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                  const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                  int32_t item_slices /* 0 = choose */, void* workspace, int64_t workspace_bytes,
                  int32_t* rank_out, int32_t* not_below_out, float* score_out, void* hip_stream);
/* bpr_rank_rows over the eligible items of an item filter (the layout, the alignment and the NULL rule: see
 * bpr_topk_rows_filtered).  Item j is eligible for row r if it is eligible for bpr_rank_rows and its bit is set;
 * everything else in the definition of rank_out, not_below_out and score_out stands.  A target whose bit is clear is
 * itself not eligible: -1 / -1 / -inf.  Scores are untouched, so the answer is what bpr_rank_rows gives on the
 * catalogue compacted to item 0 and the eligible items in ascending order (a monotone renumbering keeps the ties),
 * whatever n, the rows' order, item_slices, and however many item tiles held no eligible item and were skipped.
 * bpr_rank_workspace and bpr_rank_slices size and plan the call: the plan does not look at the filter. */
int bpr_rank_rows_filtered(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                           const int32_t* users, int64_t n,
                           const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                           const int64_t* seen_indptr /* or NULL */, const int32_t* seen_indices,
                           const uint32_t* item_filter /* [4 * ceil(I / 128)] or NULL */,
                           int32_t item_slices /* 0 = choose */, void* workspace, int64_t workspace_bytes,
                           int32_t* rank_out, int32_t* not_below_out, float* score_out, void* hip_stream);

/* ---- fold-in: user rows for users who arrive after training, learnt against the FROZEN item table (the reference
 * has no such step: its held-out users' histories are part of the training file, full-train-with-fold-in.jsonl, which
 * is why configs/RQ3/user-split has no BPR entry).  One kernel (csrc/bpr_foldin.hip); Q and item_bias are never
 * written.  The new users are the rows of a CSR — indptr [n+1] int64 (indptr[0] need not be 0: a slice of a larger
 * CSR works), items int32, sorted ascending inside a row, no duplicates, ids in [1, I) — and P_new [n, d] holds the
 * caller's initial rows on entry and the learnt rows on return.  With nnz = indptr[n] - indptr[0], row r of length m
 * takes `epochs` * m sequential SGD steps, epoch by epoch, position by position; the step of epoch e, position j has
 *     triple index   t = e * nnz + (indptr[r] - indptr[0]) + j
 *     positive       i = items[indptr[r] + j]
 *     negative       BPR_NEG_GIVEN: neg_in[t];  BPR_NEG_UNIFORM: the negative bpr_sample_uniform draws for counter
 *                    offset + t on a context whose seen row of the user is this row (same seed; no item weights);
 *                    it is also written to neg_out[t] when neg_out is not NULL
 *     update, fp32   x = <p, q_i - q_j> (+ b_i - b_j),  w = sigma(-x),  p <- p - lr (-w (q_i - q_j) + alpha_user p)
 * SKIP RULE: a triple whose negative is 0 is skipped (p unchanged) — what the sampler returns when the row covers
 * every item; so is one whose positive or given negative lies outside [1, I).  A row of length 0 keeps its initial
 * values.  The result is a pure function of these definitions: its bits do not depend on `order`, on n or on the
 * launch.  order [n] int32 or NULL: a permutation of the rows, the sequence in which they are handed to the groups of
 * the launch (longest rows first evens out the tail; NULL = list order; an entry outside [0, n) is passed over).
 * d in [1, 1024] (0: BPR_ERR_INVALID, more: BPR_ERR_UNSUPPORTED); n below 2^31; I * d and epochs * nnz below 2^31
 * (BPR_ERR_UNSUPPORTED); BPR_NEG_ADAPTIVE, BPR_NEG_DYNAMIC, BPR_NEG_WARP: BPR_ERR_UNSUPPORTED.  Arguments are validated before the device is
 * touched; n == 0 is BPR_OK.  indptr is read by the kernel only, except for ONE host read: the call copies indptr[0]
 * and indptr[n] back for the bound on epochs * nnz and waits for `hip_stream` to do so (the launch itself is
 * asynchronous; the call cannot be captured into a graph).  A device's first call allocates a few ticket words that
 * live as long as the process.  Context-free: runs on `hip_stream` of the current device. */
int bpr_fold_in_rows(const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                     const int64_t* indptr /* [n+1] */, const int32_t* items, int64_t n,
                     const int32_t* order /* [n] or NULL */,
                     int32_t epochs, float lr, float alpha_user,
                     int32_t sampler /* BPR_NEG_GIVEN | BPR_NEG_UNIFORM */,
                     const int32_t* neg_in /* [epochs*nnz], GIVEN */, int32_t* neg_out /* [epochs*nnz] or NULL */,
                     uint64_t seed, uint64_t offset,
                     float* P_new /* [n,d], in/out: the caller's initial rows */, void* hip_stream);

/* bpr_fold_in_rows with ADAPTIVE negatives (csrc/bpr_foldin_adaptive.hip).  The CSR contract, the triple index t, the
 * update, the SKIP RULE, row_order (bpr_fold_in_rows' `order`), the bounds, the one host read of indptr's ends, n == 0
 * and "validated before the device is touched; Q and item_bias are never written" are bpr_fold_in_rows'; so is the
 * purity: the bits of every output do not depend on row_order, on n, on the launch or on the seen structure the
 * kernel chooses.  What differs is the negative of triple t: it is the item bpr_sample_adaptive returns for counter
 * offset + t under `seed` and `p` (the geometric parameter, in (0, 1)) on a context whose user row is THIS row's
 * value just before that triple's update, whose seen row is this CSR row and whose snapshot is `order` / `sigma` —
 * the same device code with the (G, E) bpr_sample_adaptive dispatches for this d, so factor, rank and item agree
 * exactly.  neg_out / factor_out / rank_out [epochs * nnz] (each may be NULL) receive that call's three outputs at
 * index t.  A row with nothing unseen draws 0 and is skipped.
 * SNAPSHOT: sigma [d] fp32, the per-factor std; order [d * I] int32, column f = every item id 0..I-1 by descending
 * q_if, FULLY sorted (a partial snapshot is not accepted; the top bit of an entry is masked off and not
 * interpreted).  order needs 4 READABLE int32 BEFORE AND AFTER the array: the walk's 16-byte loads overhang a
 * column's ends by up to 3 entries, which it masks.  The pointer bpr_adaptive_snapshot_ptrs hands out satisfies
 * this.  An order entry outside [0, I) never becomes an address: it is treated as item 0 (never a candidate).
 * order and sigma are not written.  Item ids may not exceed 2^30: I - 1 > 2^30 is BPR_ERR_UNSUPPORTED; order or sigma
 * NULL and p outside (0, 1) (or NaN) are BPR_ERR_INVALID.  Context-free: runs on `hip_stream` of the current
 * device. */
int bpr_fold_in_rows_adaptive(const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                              const int32_t* order /* [d*I] */, const float* sigma /* [d] */,
                              const int64_t* indptr /* [n+1] */, const int32_t* items, int64_t n,
                              const int32_t* row_order /* [n] or NULL */,
                              int32_t epochs, float lr, float alpha_user, float p /* geometric, in (0,1) */,
                              int32_t* neg_out, int32_t* factor_out, int32_t* rank_out /* [epochs*nnz] or NULL */,
                              uint64_t seed, uint64_t offset,
                              float* P_new /* [n,d] in/out */, void* hip_stream);

/* bpr_fold_in_rows with SCORED negatives (csrc/bpr_foldin_scored.hip): dynamic negatives under BPR's loss, or the WARP
 * objective — fold new users in with the sampler the table was trained with.  The CSR contract, the triple index
 * t = e * nnz + CSR position, the counter offset + t, row_order, the bounds, the one host read of indptr's ends, n == 0
 * and "validated before the device is touched; Q and item_bias are never written" are bpr_fold_in_rows_adaptive's, and
 * so is the purity: the bits of every output do not depend on row_order, on n, on the launch or on the seen structure
 * the kernel chooses.  The triple t of the user whose row is p as it stands just before t and whose seen items are
 * its CSR row:
 *     candidates     a_1 .. a_m of bpr_sample_dynamic / bpr_sample_warp for (seed, counter offset + t, this seen row,
 *                    I, `candidates`): sample_uniform's stream, the first min(candidates, accepted) unseen ones, the
 *                    exact pick by rank when none is accepted.  No item weights: a context-free call has none.
 *     scores         x_a = <p, Q[a]> (+ item_bias[a]), fp32, by the same device code with the (G, E)
 *                    bpr_sample_dynamic dispatches for this d: picks, tries and scores agree with it exactly.
 *     BPR_NEG_DYNAMIC  the pick is bpr_sample_dynamic's (the best of a_1 .. a_m; NaN rules included), the step is
 *                    bpr_fold_in_rows': passing the picks to it as BPR_NEG_GIVEN reproduces the rows bit for bit.
 *                    A pick 0 (nothing unseen) skips the triple.  tries_out receives 0.  `margin` is ignored.
 *     BPR_NEG_WARP   violator: the smallest k with x_k > x_i - margin, tries = k;
 *                    L = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - row length;
 *                    p <- p - lr (-L (q_i - q_j) + alpha_user p)   (L where bpr_fold_in_rows has sigma(-x));
 *                    no violator among a_1 .. a_m, or a NaN x_i: the triple is SKIPPED — no step, not even the L2
 *                    term; neg_out[t] = -1, tries_out[t] = 0 (the rule of the fused STREAM path).  L = 0: the L2 term
 *                    alone.  A violator 0 (nothing unseen) is reported and not applied.
 * neg_out / tries_out [epochs * nnz] (each may be NULL) receive the pick and the tries at index t.  A positive or a
 * pick outside [1, I) skips its triple.  candidates outside 1 .. 32, and under BPR_NEG_WARP a margin that is not
 * finite and > 0: BPR_ERR_INVALID.  Any other kind: BPR_ERR_UNSUPPORTED (BPR_NEG_GIVEN, BPR_NEG_UNIFORM:
 * bpr_fold_in_rows; BPR_NEG_ADAPTIVE: bpr_fold_in_rows_adaptive).  NaN lr or alpha_user, the d and I bounds, NULLs: as
 * bpr_fold_in_rows_adaptive.  Context-free: runs on `hip_stream` of the current device. */
int bpr_fold_in_rows_scored(const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                            const int64_t* indptr /* [n+1] */, const int32_t* items, int64_t n,
                            const int32_t* row_order /* [n] or NULL */,
                            int32_t epochs, float lr, float alpha_user,
                            int32_t kind /* BPR_NEG_DYNAMIC | BPR_NEG_WARP */, int32_t candidates, float margin,
                            int32_t* neg_out /* [epochs*nnz] or NULL */, int32_t* tries_out /* [epochs*nnz] or NULL */,
                            uint64_t seed, uint64_t offset,
                            float* P_new /* [n,d] in/out */, void* hip_stream);

/* ---- item fold-in: item rows (and biases) for ITEMS that enter the catalogue after training, learnt against the
 * FROZEN user table, item table and item bias (the reference has no such step: its time-split and user-split
 * protocols put every item into the training file).  The mirror image of bpr_fold_in_rows, with its own kernel
 * (csrc/bpr_foldin_items.hip): every triple of a new item meets a different user, and its negative must be unseen by
 * THAT user.  P, Q, item_bias and the seen CSR are never written.  The new items are the rows of a CSR — indptr [m+1]
 * int64 (indptr[0] need not be 0: a slice of a larger CSR works), users int32, sorted ascending inside a row, no
 * duplicates, ids in [0, U) — and Q_new [m, d] (with bias_new [m]) holds the caller's initial rows on entry and the
 * learnt rows on return.  With nnz = indptr[m] - indptr[0], row r of length L takes `epochs` * L sequential SGD steps,
 * epoch by epoch, position by position; the step of epoch e, position k has
 *     triple index   t = e * nnz + (indptr[r] - indptr[0]) + k
 *     user           u = users[indptr[r] + k]
 *     negative       BPR_NEG_GIVEN: neg_in[t];  BPR_NEG_UNIFORM: exactly the item bpr_sample_uniform draws for user u
 *                    at counter offset + t under `seed` on a context whose seen CSR is (seen_indptr [U+1],
 *                    seen_indices) (no item weights); it is also written to neg_out[t] when neg_out is not NULL.
 *                    Both seen pointers NULL: nothing is seen besides item 0; one NULL and one not: BPR_ERR_INVALID.
 *                    Negatives come from the frozen table only, [1, I): a new item is never a negative.
 *     update, fp32   x = <p_u, q - q_j> (+ b - b_j),  w = sigma(-x),  q <- q - lr (-w p_u + alpha_item q),
 *                    b <- b + lr w   (q, b: the row being learnt; the bias has no L2, as Model.regularization has none)
 * item_bias and bias_new are both NULL (no bias term) or both given; anything else is BPR_ERR_INVALID.
 * SKIP RULE: a triple whose negative is 0 is skipped (q and b unchanged) — what the sampler returns for a user who has
 * seen every item; so is one whose user lies outside [0, U) (its neg_out entry is 0) or whose given negative lies
 * outside [1, I).  A row of length 0 keeps its initial values.  The result is a pure function of these definitions:
 * the bits of Q_new, bias_new and neg_out do not depend on `order`, on m or the other rows, on the launch or on the
 * kernel's prefetch depth.  order [m] int32 or NULL: as bpr_fold_in_rows' (an entry outside [0, m) is passed over).
 * d in [1, 1024] (0: BPR_ERR_INVALID, more: BPR_ERR_UNSUPPORTED); m below 2^31; I * d, U * d and epochs * nnz below
 * 2^31 (BPR_ERR_UNSUPPORTED); BPR_NEG_ADAPTIVE, BPR_NEG_DYNAMIC, BPR_NEG_WARP: BPR_ERR_UNSUPPORTED; NaN lr or alpha_item: BPR_ERR_INVALID.  Arguments
 * are validated before the device is touched; m == 0 is BPR_OK.  indptr is read by the kernel only, except for ONE
 * host read, bpr_fold_in_rows': the call copies indptr[0] and indptr[m] back for the bound on epochs * nnz and waits
 * for `hip_stream` to do so (the launch itself is asynchronous; the call cannot be captured into a graph).  It shares
 * bpr_fold_in_rows' ticket words.  Context-free: runs on `hip_stream` of the current device. */
int bpr_fold_in_item_rows(const float* P, int64_t U, const float* Q, const float* item_bias /* or NULL */,
                          int64_t I, int32_t d,
                          const int64_t* seen_indptr /* [U+1] or NULL */, const int32_t* seen_indices,
                          const int64_t* indptr /* [m+1] */, const int32_t* users, int64_t m,
                          const int32_t* order /* [m] or NULL */,
                          int32_t epochs, float lr, float alpha_item,
                          int32_t sampler /* BPR_NEG_GIVEN | BPR_NEG_UNIFORM */,
                          const int32_t* neg_in /* [epochs*nnz], GIVEN */, int32_t* neg_out /* [epochs*nnz] or NULL */,
                          uint64_t seed, uint64_t offset,
                          float* Q_new /* [m,d] in/out */, float* bias_new /* [m] in/out, or NULL */,
                          void* hip_stream);

/* bpr_fold_in_item_rows in BOTH roles (csrc/bpr_foldin_items_roles.hip): besides being the positive of its audience's
 * triples, a new item is the NEGATIVE of neg_role (R >= 0) training interactions per epoch — triples (u, i, new) where
 * (u, i) is a training interaction of a user outside the item's audience, the triples that would have drawn it in joint
 * training with uniform negatives (about T / I per epoch for every item, whence one R for all rows).  Every argument it
 * shares with bpr_fold_in_item_rows means what it means there; so do the CSR contract, `order`, the limits, "validated
 * before the device is touched", the one host read, the ticket words, m == 0 and what is never written — to which
 * train_users / train_items (int32 [T], T < 2^31, as the trainers take them; never written) are added.
 * STEP ORDER.  Row r of length L takes `epochs` passes of L + R sequential steps.  Step s in [0, L + R) of a pass is a
 * negative-role step iff floor((s + 1) R / (L + R)) > floor(s R / (L + R)) (64-bit integers); rho = floor(s R / (L + R))
 * negative-role steps precede it, and a positive-role step has position k = s - rho.  A row of length 0 takes R
 * negative-role steps per epoch when R > 0 and keeps its initial values when R = 0.
 * POSITIVE-ROLE STEP (e, k): exactly bpr_fold_in_item_rows' step — its triple index t, counter offset + t, neg_in /
 * neg_out entry t, skip rule and update.  With R = 0 the call returns bpr_fold_in_item_rows' bits for Q_new, bias_new
 * and neg_out.
 * NEGATIVE-ROLE STEP (e, rho), with g = (e * m + r) * R + rho:
 *     attempts       a = 0 .. 15, in order: w_a = word a & 3 of the Philox4x32-10 block with counter words (lo32(c),
 *                    hi32(c), a >> 2, 2), c = offset + g, under the key (lo32(seed), hi32(seed)).  Counter word 3 = 2
 *                    separates the stream from the uniform sampler's (0: candidates and rank pick) and the adaptive
 *                    sampler's (1).  tau = (uint64) w_a * T >> 32, u = train_users[tau], i = train_items[tau]; the
 *                    attempt is accepted iff 0 <= u < U, 1 <= i < I and u is not in row r's audience.
 *     interaction    that of the first accepted attempt; role_out[g] = its tau.  None accepted (a row whose audience is
 *                    nearly everyone): the step is skipped, role_out[g] = -1, q and b unchanged.
 *     update, fp32   x = <p_u, q_i - q> (+ b_i - b),  w = sigma(-x),  q <- q - lr (w p_u + alpha_item q),
 *                    b <- b - lr w
 * Both updates form x as bpr_fold_in_item_rows does: per lane an fmaf chain from 0.0f over its elements of p_u times the
 * difference, the group's sum of the lanes, then the bias difference added; w = 1 / (1 + exp(x)).
 * role_out [epochs * m * R] int32 or NULL; the entries of rows that `order` passes over are not written.  The result is
 * a pure function of these definitions: the bits of Q_new, bias_new, neg_out and role_out do not depend on `order`, on
 * the launch or on the kernel's prefetch depth; a row's bits depend on m and r only through g.
 * neg_role < 0, or neg_role > 0 with train_users or train_items NULL or T < 1: BPR_ERR_INVALID (neg_role = 0 accepts NULL
 * arrays).  epochs * m * neg_role, and epochs * (nnz + m * neg_role) (the kernel's 32-bit step counters), must be below
 * 2^31: BPR_ERR_UNSUPPORTED. */
int bpr_fold_in_item_rows_roles(const float* P, int64_t U, const float* Q, const float* item_bias /* or NULL */,
                                int64_t I, int32_t d,
                                const int64_t* seen_indptr /* [U+1] or NULL */, const int32_t* seen_indices,
                                const int64_t* indptr /* [m+1] */, const int32_t* users, int64_t m,
                                const int32_t* order /* [m] or NULL */,
                                int32_t epochs, float lr, float alpha_item,
                                int32_t sampler /* BPR_NEG_GIVEN | BPR_NEG_UNIFORM */,
                                const int32_t* neg_in /* [epochs*nnz], GIVEN */,
                                int32_t* neg_out /* [epochs*nnz] or NULL */,
                                uint64_t seed, uint64_t offset,
                                const int32_t* train_users /* [T] */, const int32_t* train_items /* [T] */, int64_t T,
                                int32_t neg_role /* R */, int32_t* role_out /* [epochs*m*R] or NULL */,
                                float* Q_new /* [m,d] in/out */, float* bias_new /* [m] in/out, or NULL */,
                                void* hip_stream);

/* ---- neighbours: the k rows of a table most similar to each of a list of query rows ("items like this one",
 * "users like this one"; the reference has no such call).  One fused kernel (csrc/bpr_neighbors.hip) with
 * bpr_topk_rows' tiling and selection, and no [n, N] buffer anywhere.  Query r is the row X[rows[r]] ([*, d] fp32
 * row-major; X may be T itself or another table of the same d, e.g. freshly folded-in rows), the table is T [N, d].
 *
 * Scores.  dot(x, t) is the fp32 fmaf chain of bpr_topk_rows over the features in its fixed order (per 8 features:
 * 0, 4, 1, 5, 2, 6, 3, 7, from 0.0f), without a bias.
 *   BPR_SIM_DOT     s(r, j) = dot(X[rows[r]], T[j]).  With X = P, exclude = NULL and first = 1 the output equals
 *                   bpr_topk_rows' without a bias and without a seen CSR, bit for bit.
 *   BPR_SIM_COSINE  ss(v) = dot(v, v): ONE fp32 chain ss = fmaf(v_f, v_f, ss) from 0.0f over the d features in
 *                   dot's order (per 8 features: 0, 4, 1, 5, 2, 6, 3, 7).
 *                   rn(v) = 1.0f / sqrt(ss(v)): the IEEE-754 correctly rounded fp32 square root, then the correctly
 *                   rounded fp32 division (CUDA's __fdiv_rn(1.0f, __fsqrt_rn(ss)); numpy's float32 arithmetic).
 *                   s(r, j) = (dot(x, t) * rn(t)) * rn(x): two fp32 multiplications in that order.
 *                   A pre-pass kernel writes rn of the N table rows and the n queries into the workspace on every
 *                   call; nothing is cached between calls.
 * Eligibility.  Row j of T is eligible for query r if first <= j < N, j != exclude[r] (exclude NULL or exclude[r] <
 * 0: no row is left out) and, under cosine, ss(T[j]) > 0 (a NaN fails that comparison, so a row with a NaN is never
 * returned; so is an all-zero row.  Under BPR_SIM_DOT a zero row is eligible, with score 0).  Under cosine a query with
 * !(ss > 0) gets a fully padded row.
 * Output.  ids_out / scores_out [n, k]: the eligible rows sorted by score descending, ties by ascending id; a query
 * with fewer than k eligible rows ends in id -1 / score -inf.  A NaN score is never better than anything, the initial
 * threshold included: it is never returned, and the row may end in padding although rows of T are left.  +inf and
 * -inf scores are ordered like any other, and a real row scoring -inf keeps its id.  Under cosine an ss that
 * overflowed is +inf > 0: rn = +0, the row stays eligible and its scores are +-0 or (inf * 0) NaN.
 * The result is a pure function of the inputs: its bits do not depend on n, on a query's place in the list (which may
 * repeat rows) or on item_slices (0 = the library chooses; s > 1 cuts the table over s workgroups per query tile, for
 * lists too short to fill the chip, and needs the workspace).  d in [1, 1024], 1 <= k <= 128, item_slices in [0, 64],
 * N in [1, 2^31), n < 2^31, first >= 0, a known metric: anything else is BPR_ERR_INVALID.  `rows` are not checked
 * against X.  Arguments are validated before the device is touched; n == 0 is BPR_OK.  Context-free: runs on
 * `hip_stream` of the current device. */
#define BPR_SIM_DOT 0
#define BPR_SIM_COSINE 1
/* bytes of device workspace bpr_neighbors_rows needs for this shape: the slices' partial results as
 * bpr_topk_workspace counts them (0 with one slice; with s slices s * n * k * 8; item_slices 0: never less than for a
 * smaller n), plus (N + n) * 4 under BPR_SIM_COSINE */
int bpr_neighbors_workspace(int64_t n, int64_t N, int32_t d, int32_t k, int32_t metric, int32_t item_slices,
                            int64_t* bytes_host);
/* the slice count a call of this shape runs with (as bpr_topk_slices: passing it back as item_slices makes
 * bpr_neighbors_workspace answer exactly that call's need) */
int bpr_neighbors_slices(int64_t n, int64_t N, int32_t d, int32_t k, int32_t item_slices, int32_t* slices_host);
int bpr_neighbors_rows(const float* X, const float* T, int64_t N, int32_t d,
                       const int32_t* rows, int64_t n,           /* query r is X[rows[r]] */
                       const int32_t* exclude /* [n] or NULL */, /* id of T left out of row r; < 0: none */
                       int32_t first,                            /* ids of T below `first` are never returned */
                       int32_t metric, int32_t k, int32_t item_slices /* 0 = choose */,
                       void* workspace, int64_t workspace_bytes,
                       int32_t* ids_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);
/* bpr_neighbors_rows over the rows of T whose bit is set in a filter over T's N rows (the layout of
 * bpr_topk_rows_filtered: 4 * ceil(N / 128) words, 16-byte aligned, NULL = the unfiltered call itself).  Eligibility
 * gains "bit j set"; `first` (the filter's lower bound: with first = 0 row 0 is a row like any other and its bit
 * counts), `exclude` and the cosine rule are unchanged, and so is every score: the result is bpr_neighbors_rows' on
 * the eligible rows of T alone, ids mapped back, k ids where filtering after the cut returns fewer.  The cosine
 * pre-pass still writes the norms of all N rows.  bpr_neighbors_workspace and bpr_neighbors_slices are the call's. */
int bpr_neighbors_rows_filtered(const float* X, const float* T, int64_t N, int32_t d,
                                const int32_t* rows, int64_t n, const int32_t* exclude /* [n] or NULL */,
                                int32_t first, int32_t metric,
                                const uint32_t* item_filter /* [4 * ceil(N / 128)] or NULL */,
                                int32_t k, int32_t item_slices /* 0 = choose */,
                                void* workspace, int64_t workspace_bytes,
                                int32_t* ids_out /* [n,k] */, float* scores_out /* [n,k] */, void* hip_stream);

/* ---- re-ranking: the k best of a GIVEN candidate list per row, and the score of every candidate ("score this user
 * on these items": availability filters, second-stage re-ranking, sampled-negative protocols, explicit pairs).  The
 * reference has no candidate path: it ranks through full logits (example.py:195-230), which this replaces for a
 * narrowed catalogue.  One fused gather kernel (csrc/bpr_rerank.hip): no [nnz, d] buffer, no sweep of the item table,
 * no workspace.
 * Rows.  Row r is user users[r] with the candidates cand_items[cand_indptr[r] .. cand_indptr[r + 1]) (cand_indptr
 * [n + 1] int64, non-decreasing; unsorted, duplicates allowed, any length including 0), or — cand_indptr NULL — the
 * ONE list cand_items[0 .. shared_len) for every row.  With a cand_indptr, shared_len is only a hint to the launch
 * plan: a typical row length (nnz / n), 0 = unknown; it changes no output.
 * Eligibility.  A candidate is eligible if 0 < id < I and id is not in the user's row of the seen CSR (seen_indptr
 * [U + 1] int64, seen_indices int32 sorted per row, as bpr_bind_seen_csr; both NULL: nothing is seen).  It is decided
 * before the item row is read: an ineligible candidate costs no table traffic.
 * Scores.  s(u, i) = bpr_topk_rows' / bpr_rank_rows' / bpr_neighbors_rows' (dot) score, bit for bit: one fp32 fmaf
 * chain from 0.0f over the features in the fixed order (per 8 features: 0, 4, 1, 5, 2, 6, 3, 7), then item_bias[i]
 * as one fp32 add.  A table that is not finite gives IEEE's infinities and NaNs: cand_scores_out holds them as they
 * are; in items_out a NaN score is never returned (the row may end in padding), +-inf scores are ordered like any
 * other and a real candidate scoring -inf keeps its id.
 * Output.  cand_scores_out (may be NULL if k > 0), aligned with the candidates ([n, shared_len] row-major for the
 * shared list): the score, -inf for an ineligible candidate.  With k > 0, items_out / scores_out [n, k]: the
 * eligible candidates sorted by score descending, ties by ascending id; an id listed m times is a candidate m times
 * and may be returned m times, adjacent; a row with fewer than k eligible candidates ends in id -1 / score -inf.
 * k == 0 writes cand_scores_out only.
 * The result is a pure function of the inputs: its bits do not depend on n, on a row's place in the call, on the
 * order of the candidates inside a row (cand_scores_out moves with them) or on `layout` (0 = the library chooses;
 * 1 = a wave of 64 lanes per row, 2 = a workgroup of 256 threads per row).  A row is never split over workgroups.
 * d in [1, 1024], 0 <= k <= 128, I in [1, 2^31), n >= 0, shared_len >= 0, layout in [0, 2], k == 0 only with
 * cand_scores_out, the seen pointers both NULL or both given: anything else is BPR_ERR_INVALID.  users, cand_indptr
 * and seen_indptr are read unchecked by the kernel; candidate ids are checked.  Arguments are validated before the
 * device is touched; n == 0 is BPR_OK.  Nothing is read back: the call is asynchronous and can be captured into a
 * graph.  Context-free: runs on `hip_stream` of the current device. */
int bpr_rerank_rows(const float* P, const float* Q, const float* item_bias /* or NULL */, int64_t I, int32_t d,
                    const int32_t* users, int64_t n,
                    const int64_t* cand_indptr /* [n+1] or NULL */, const int32_t* cand_items, int64_t shared_len,
                    const int64_t* seen_indptr /* [U+1] or NULL */, const int32_t* seen_indices,
                    int32_t k, int32_t layout /* 0 = choose */,
                    float* cand_scores_out /* or NULL */, int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */,
                    void* hip_stream);
/* the layout (1 or 2) and the tile (candidates a team stages at a time: 64 or 256) a call of this shape runs with;
 * row_len is what the call passes as shared_len */
int bpr_rerank_layout(int64_t n, int32_t d, int32_t k, int64_t row_len, int32_t layout, int32_t* layout_host,
                      int32_t* tile_host);

/* ---- diversified top-k: greedy maximal marginal relevance (MMR) over a pool of candidates per row — "the k best,
 * but not k copies of one thing".  The reference has no such pass: it ranks through full logits (example.py:195-230).
 * The input is what bpr_topk_rows / bpr_rerank_rows return ([n, C] ids and scores, -1 / -inf padding); the output has
 * the same form.  One fused kernel (csrc/bpr_diversify.hip): a workgroup per row keeps the row's C x C similarities in
 * LDS; no [n, C, d] gather, no [n, C, C] matrix, no workspace.
 * Rows.  Row r has the C candidates cand_items[r, 0 .. C) (int32) with relevances cand_scores[r, 0 .. C) (fp32),
 * row-major, 1 <= C <= 128; the item table is Q [I, d] fp32 row-major.
 * Eligibility.  A candidate is eligible if 0 < id < I and its relevance is finite (this drops the -1 / -inf padding,
 * id 0 and a NaN relevance).  It is decided before the item row is read: an ineligible candidate costs no table
 * traffic.  An id listed m times is m candidates.
 * Similarity.  dot(a, b) is bpr_topk_rows' chain on the two item rows: ONE fp32 accumulator from +0.0f, one fmaf per
 * feature in the fixed order (per 8 features: 0, 4, 1, 5, 2, 6, 3, 7), every chunk of 32 features run to its end over
 * zeros past d — the bits bpr_rerank_rows' cand_scores_out holds for P = Q, user a, candidate b, no bias.
 *   BPR_SIM_DOT     sim(a, b) = dot(a, b).
 *   BPR_SIM_COSINE  sim(a, b) = dot(a, b) * (rn(a) * rn(b)): two fp32 multiplications in THAT association, with
 *                   rn(v) = 1.0f / sqrt(dot(v, v)), the correctly rounded fp32 square root and division (as
 *                   bpr_neighbors_rows' rn).  A row with !(dot(v, v) > 0) has similarity 0 to everything.  This is
 *                   NOT bpr_neighbors_rows' (dot * rn(t)) * rn(x): here sim(a, b) and sim(b, a) are the same bits.
 * Relevance.  BPR_SCALE_NONE: rel' = rel.  BPR_SCALE_MINMAX: rel' = (rel - lo) / (hi - lo) with lo / hi the smallest /
 * largest relevance of the row's eligible candidates: fp32 subtraction, subtraction, correctly rounded division;
 * hi == lo: rel' = 0.  The scores returned are always the ORIGINAL relevances.
 * Objective.  oml = 1.0f - lam (fp32); m(c) = the largest sim(c, s) over the candidates s picked so far (after the
 * first pick it is that similarity, negative or not; 0.0f while nothing is picked);
 *   v(c) = (lam * rel'(c)) - (oml * m(c)): three separately rounded fp32 operations, no fma.
 * Each step picks the unpicked eligible candidate with the largest v; ties go to the larger original relevance, then
 * the smaller id, then the smaller position: the output is a function of the multiset of (id, relevance) pairs of the
 * row.  A NaN v (tables are taken to be finite; an overflowing dot can make one) counts, and is reported, as -inf.
 * Output.  items_out / scores_out [n, k] in pick order, and — mmr_out may be NULL — the v each pick won with; a row
 * with fewer than k eligible candidates ends in id -1 / score -inf / mmr -inf.
 * The result is a pure function of the inputs: its bits do not depend on n, on a row's place in the call, on the order
 * of the candidates inside a row or on `layout` (0 = the library chooses; 1 = a workgroup of 256 threads per row, the
 * only layout today).  1 <= C <= 128, 0 <= k <= 128, d in [1, 1024], I in [1, 2^31), n >= 0, 0 <= lam <= 1 (a NaN is
 * refused), a known metric and scale, layout in [0, 1]: anything else is BPR_ERR_INVALID.  Arguments are validated
 * before the device is touched; n == 0 and k == 0 are BPR_OK without tables.  Nothing is read back: the call is
 * asynchronous and can be captured into a graph.  Context-free: runs on `hip_stream` of the current device. */
#define BPR_SCALE_NONE 0
#define BPR_SCALE_MINMAX 1
int bpr_diversify_rows(const float* Q, int64_t I, int32_t d,
                       const int32_t* cand_items /* [n,C] */, const float* cand_scores /* [n,C] */, int64_t n,
                       int32_t C, int32_t k, float lam, int32_t metric /* BPR_SIM_* */, int32_t scale /* BPR_SCALE_* */,
                       int32_t layout /* 0 = choose */,
                       int32_t* items_out /* [n,k] */, float* scores_out /* [n,k] */, float* mmr_out /* [n,k] or NULL */,
                       void* hip_stream);
/* what a call of this shape runs with: the layout (1), the pool padded to a multiple of 32 and the bytes of LDS a
 * workgroup holds (they depend on C only: 9,344 / 22,784 / 40,448 / 62,336 at C <= 32 / 64 / 96 / 128) */
int bpr_diversify_layout(int64_t n, int32_t C, int32_t k, int32_t layout, int32_t* layout_host, int32_t* cpad_host,
                         int64_t* lds_host);

/* ---- multi-GPU item-table reconciliation (no reference counterpart: the reference's DDP path is
 * never enabled by a config, experiments/launcher.py:35-73).  The all-reduce itself is RCCL via
 * torch.distributed; these two fused elementwise kernels bracket it (revisit_bpr/distributed.py).
 * Context-free: arrays of n floats and the HIP stream to run on. */
/* own[k] = tot[k] = q[k] - base[k]   (this rank's delta since the last reconciliation) */
int bpr_item_delta(const float* q, const float* base, float* own, float* tot, int64_t n,
                   void* hip_stream);
/* tot = all-reduced sum of every rank's delta.  base += scale*tot (bit-identical on every rank);
 * rebase == 0: q += scale*tot - own   (asynchronous: q keeps what it learned since bpr_item_delta)
 * rebase == 1: q  = base              (blocking reconcile: every replica becomes the same cut) */
int bpr_item_fold(float* q, float* base, const float* own, const float* tot, float scale,
                  int32_t rebase, int64_t n, void* hip_stream);
/* bpr_item_fold (rebase = 0) immediately followed by bpr_item_delta, as one pass over the table:
 * the per-period reconciliation step when nothing trains between folding the previous all-reduce
 * and cutting the next delta.  tot holds the all-reduced sum on entry and the new delta on exit. */
int bpr_item_fold_delta(float* q, float* base, float* own, float* tot, float scale, int64_t n,
                        void* hip_stream);

/* ---- measurement --------------------------------------------------------------------------- */
/* Average duration (ms) of the dominant kernel over the launches recorded since the last reset,
 * measured with hipEvents on the ctx stream (bench.py's roofline.achieved uses this).
 * bpr_timing_enable(ctx, N) turns recording on for every N-th launch (N >= 1; 0 = off).  The two
 * event records around a timed launch cost ~6 us of stream idle time each on MI355X — ~4 % of a
 * 0.3 ms step when every launch is timed — so bench.py samples every 8th launch of the timed region. */
int bpr_timing_enable(bpr_ctx* ctx, int32_t on);
int bpr_timing_read_host(bpr_ctx* ctx, double* avg_ms_host, int64_t* launches_host);

#ifdef __cplusplus
}
#endif
#endif /* BPRCORE_H */
