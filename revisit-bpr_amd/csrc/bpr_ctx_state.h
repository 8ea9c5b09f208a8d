// bpr_ctx_state.h — the cross-call state of a bpr_ctx: the ONLY place where these fields are assigned.  Each function
// is one event in the life of a ctx; an entry point says what happened, not which flags follow from it.
//
//   keys_cut         true iff keysT holds the keys of Q (+ hot block) as they are now: the next refresh only sorts.
//                    set: keys_were_cut (a cut launch's epilogue, the asynchronous cut, bpr_sync_cut);
//                    cleared: items_moved (whatever writes Q, or frees keysT), keys_consumed (a refresh took them)
//   keys_event       (read only while keys_cut) true iff ev_keys rides on the cut kernel itself, so a split refresh
//                    need not record it.  set / cleared with keys_cut: keys_were_cut, keys_consumed
//   keys_on_side     (read only while keys_cut) true iff that cut ran on c->side: a sort on c->stream waits for ev_keys.
//                    set: keys_were_cut(on_side); cleared: keys_consumed
//   acut_pending     true iff a cut on c->side may still read Q, the hot deltas and a launch's partials.
//                    set: keys_were_cut(on_side); cleared: acut_waited (c->stream now waits for ev_keys)
//   keys_front_stale true iff a cut has overwritten the key buffer the partial FRONT snapshot was sorted from: it can
//                    be neither walked nor completed.  set: keys_were_cut; cleared: front_replaced (a snapshot swap)
//   refresh_pending  true iff a split refresh's sort is queued on c->side and not committed.
//                    set: split_refresh_queued; cleared: split_refresh_done (commit, or the buffers freed)
//   hot_unfolded     true iff the hot block holds deltas that the read-only asynchronous cut (acut_fold = 0) left:
//                    Q alone is not the item table.  set: acut_left_unfolded; cleared: hot_block_folded
//   hot_uncut        true iff, under the hot tier, the block holds deltas of a launch that no exchange has taken out:
//                    the LDS-tier kernel must not run.  set: launch_left_hot_deltas; cleared: hot_block_cut
//                    (bpr_hot_exchange with cut = 1, bpr_sync_cut, the block freed)
//   defer_pending    true iff c->dev_scalars holds defer_blocks loss partials of a hot-tier cut launch, owed to
//   (+ defer_blocks, defer_out (the caller's scalars).  set: stats_deferred; cleared: stats_taken (bpr_sync_cut sums
//    defer_out)      them in its pass, flush_deferred_stats for whoever comes first instead)
//   bias_w_valid     true iff bias_w (one item per line) equals the dense vector bias_w_of: a tracked launch skips the
//   (+ bias_w_of)    refill.  set: bias_wide_synced (a launch's write-back); cleared: bias_wide_taken (a launch works on
//                    it), bias_moved (somebody else writes the item_bias, or says so: bpr_bias_written)
#pragma once
#include "bpr_ctx.h"

namespace bpr {

// something wrote Q (or will before the next refresh), or the key buffers were freed: keysT is not Q's keys
inline void items_moved(bpr_ctx* c) { c->keys_cut = false; }
// something wrote item_bias outside a STREAM launch
inline void bias_moved(bpr_ctx* c) { c->bias_w_valid = false; }

// c->keysT holds the next snapshot's keys.  by_event: ev_keys rides on the cut kernel; on_side: the cut runs on
// c->side — whoever sorts these keys on the launch stream waits for ev_keys, and so does a launch outside the acut
// pipeline (the cut reads Q and that launch's partials).  stales_front = false: bpr_sync_cut, which has never marked
// the front (reachable — cut, begin, commit, cut, begin, cut with partial snapshots — and kept as it is: DESIGN.md)
inline void keys_were_cut(bpr_ctx* c, bool by_event, bool on_side, bool stales_front = true) {
  c->keys_cut = true;
  if (stales_front && c->meta_front != nullptr && c->keysT == c->keys_front) c->keys_front_stale = true;
  c->keys_event = by_event;
  if (on_side) c->keys_on_side = c->acut_pending = true;
}
// a refresh took the keys (or cut its own): the next cut goes to the other buffer
inline void keys_consumed(bpr_ctx* c) { c->keys_cut = c->keys_event = c->keys_on_side = false; }
// c->stream waits for ev_keys: the asynchronous cut is over before anything queued from here on
inline void acut_waited(bpr_ctx* c) { c->acut_pending = false; }
// a snapshot became the front one
inline void front_replaced(bpr_ctx* c) { c->keys_front_stale = false; }
inline void split_refresh_queued(bpr_ctx* c) { c->refresh_pending = true; }
inline void split_refresh_done(bpr_ctx* c) { c->refresh_pending = false; }

// a hot-tier launch: its deltas stay in the block for bpr_hot_exchange / bpr_sync_cut
inline void launch_left_hot_deltas(bpr_ctx* c) { c->hot_uncut = true; }
// the block is zero again (or gone): the next launch may take the LDS tier
inline void hot_block_cut(bpr_ctx* c) { c->hot_uncut = false; }
// the read-only asynchronous cut left this launch's deltas (if it has a hot block) beside Q
inline void acut_left_unfolded(bpr_ctx* c, bool hot) { c->hot_unfolded = hot; }
inline void hot_block_folded(bpr_ctx* c) { c->hot_unfolded = false; }

// a cut launch under the hot tier leaves `blocks` loss partials in c->dev_scalars, owed to `out`
inline void stats_deferred(bpr_ctx* c, int blocks, float* out) {
  c->defer_blocks = blocks;
  c->defer_out = out;
  c->defer_pending = true;
}
inline void stats_taken(bpr_ctx* c) {
  c->defer_pending = false;
  c->defer_out = nullptr;
}

// (re)fill the wide table — unless it is known to equal the dense vector still: the epilogue of the previous launch
// wrote it back, and nobody has touched the vector since (every entry point of the library that writes it says so;
// writes of the caller's own: bpr_bias_written)
inline bool bias_wide_refill_needed(const bpr_ctx* c) {
  return !(c->bias_track && c->bias_w_valid && c->bias_w_of == c->bias);
}
// a launch works on the wide table: the dense vector lags until the write-back
inline void bias_wide_taken(bpr_ctx* c) {
  c->bias_w_valid = false;
  c->bias_w_of = c->bias;
}
// the write-back is queued: dense == wide again once it has run
inline void bias_wide_synced(bpr_ctx* c) { c->bias_w_valid = true; }

}  // namespace bpr
