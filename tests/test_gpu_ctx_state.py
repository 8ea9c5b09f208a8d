"""Transitions of the ctx's cross-call state (csrc/bpr_ctx_state.h) that no other test holds: a short call sequence
at the smallest shape that reaches the state, against the same sequence with the state forced the slow way.

Shapes: U = 64, I = 320, d = 32 (the LDS tier needs d = G * E), 2,048 triples per launch, 16 hot rows.  Launches run
with max_inflight = 1 and given negatives, so both sequences run the same kernels on the same values in the same order
on one stream: equality is exact.

Found by emptying each function of bpr_ctx_state.h in turn.  Held elsewhere, by tests/test_gpu_parity.py: bias_moved,
launch_left_hot_deltas, acut_left_unfolded, split_refresh_queued, split_refresh_done.  Held here: items_moved,
keys_consumed, keys_were_cut, front_replaced, hot_block_cut, hot_block_folded, stats_deferred, stats_taken,
bias_wide_taken, bias_wide_synced.  acut_waited emptied IS the slow way (every launch outside the acut pipeline waits
once more for an event that has fired): no sequence of calls tells it from the fast way by its results.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U, I, D, N, H = 64, 320, 32, 2048, 16


@pytest.fixture(scope="module")
def problem():
    rng = np.random.default_rng(11)
    P = rng.normal(0, 0.2, (U, D)).astype(np.float32)
    Q = rng.normal(0, 0.2, (I, D)).astype(np.float32)
    b = rng.normal(0, 0.1, I).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b[0] = 0
    users = np.sort(rng.integers(1, U, 3 * N)).astype(np.int32)
    pos = (1 + (rng.zipf(1.4, 3 * N) % (I - 1))).astype(np.int32)
    neg = rng.integers(1, I, 3 * N).astype(np.int32)
    return P, Q, b, users, pos, neg


def _engine(problem, bias, items=I):
    from revisit_bpr import engine as eng

    P, Q, b, users, pos, neg = problem
    if items != I:  # a wider item table over the same triples (partial snapshots need 2,048 columns' keys)
        Q = np.random.default_rng(12).normal(0, 0.2, (items, D)).astype(np.float32)
    dev = torch.device("cuda")
    e = eng.Engine(torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev),
                   torch.from_numpy(b).to(dev) if bias else None)
    e.set_reg(0.01, 0.02, 0.03)
    e.set_optimizer(eng.OPT_SGD, lr=0.05)
    e.set_stream_opts(True, 0)
    return e, [torch.from_numpy(x).to(dev) for x in (users, pos, neg)]


def _launch(e, ids, k, **kw):
    from revisit_bpr import engine as eng

    u, p, n = (x[k * N:(k + 1) * N] for x in ids)
    e.train_stream(u, p, sampler=eng.NEG_GIVEN, neg=n, max_inflight=1, **kw)


def _hot_set(e, ids):
    counts = torch.bincount(ids[1].long(), minlength=e.I)
    hot = torch.argsort(counts, descending=True)[:H].to(torch.int32)
    e.set_hot_items(hot.cpu(), counts.cpu())


def test_a_new_hot_set_lets_the_lds_tier_run_again(problem):
    """hot_block_cut in hot_free: under the hot tier a launch leaves its deltas in the block (hot_uncut), which keeps
    the LDS-tier kernel out; a new hot set is a new, zeroed block, so the next launch may take the LDS tier — as it
    does on an engine that never entered the tier."""
    rows = []
    for tier in (True, False):
        e, ids = _engine(problem, bias=False)
        _hot_set(e, ids)
        e.set_hot_lds(H, always=True)
        if tier:
            hb = torch.zeros(H, D, device=e.Q.device)
            e.hot_tier_begin(hb)
            _launch(e, ids, 0)
            assert e.stream_lds_rows() > 0  # the block was clean
            _launch(e, ids, 1)
            assert e.stream_lds_rows() == 0  # the first launch's deltas are still in it
            e.hot_tier_end()
            _hot_set(e, ids)
        _launch(e, ids, 2)
        rows.append(e.stream_lds_rows())
        e.close()
    assert rows[0] == rows[1] > 0


def test_a_refresh_cuts_its_own_keys_once_the_table_has_moved(problem):
    """items_moved and keys_consumed: a cut launch leaves the next snapshot's keys behind, and the next refresh only
    sorts them — unless the table has moved since (a plain launch: items_moved), or a refresh has already taken them
    (keys_consumed; then the caller scales Q through torch, which the library cannot see).  Forced the slow way: a
    second refresh, which always cuts its own keys, gives the same snapshot; and sigma of 2 Q is exactly 2 sigma."""
    from revisit_bpr import engine as eng

    e, ids = _engine(problem, bias=False)
    u, p, n = (x[:N] for x in ids)
    e.train_stream(u, p, sampler=eng.NEG_GIVEN, neg=n, max_inflight=1, cut=True)
    _launch(e, ids, 1)  # the table moves after the cut
    e.adaptive_refresh()
    order1, sigma1 = (t.clone() for t in e.adaptive_snapshot())
    e.adaptive_refresh()
    order2, sigma2 = (t.clone() for t in e.adaptive_snapshot())
    assert torch.equal(order1, order2) and torch.equal(sigma1, sigma2)
    e.train_stream(u, p, sampler=eng.NEG_GIVEN, neg=n, max_inflight=1, cut=True)
    e.adaptive_refresh()  # takes the keys of the cut
    sigma3 = e.adaptive_snapshot()[1].clone()
    e.Q.mul_(2.0)
    e.adaptive_refresh()
    assert torch.equal(e.adaptive_snapshot()[1], 2.0 * sigma3)
    e.close()


def test_a_folded_hot_block_lets_the_lds_tier_run_again(problem):
    """hot_block_folded: the read-only asynchronous cut (acut_fold = 0) leaves its launch's deltas in the hot block,
    which keeps the LDS-tier kernel out; once somebody has folded them (bpr_hot_fold) the next launch takes the LDS
    tier — as it does on an engine that folded after every launch."""
    rows = []
    for acut in (True, False):
        e, ids = _engine(problem, bias=False)
        _hot_set(e, ids)
        e.set_hot_lds(H, always=True)
        if acut:
            e.set_tuning("acut_fold", 0)
            _launch(e, ids, 0, cut="async")
            e.hot_fold()
        _launch(e, ids, 1)
        rows.append(e.stream_lds_rows())
        e.close()
    assert rows[0] == rows[1] > 0


def test_deferred_statistics_arrive_once_whoever_takes_them(problem):
    """stats_deferred and stats_taken: a cut launch under the hot tier leaves its loss partials to the bpr_sync_cut
    that follows; the slow way is bpr_hot_exchange, which sums them with a kernel of their own.  Either way they arrive
    once: the launch after must not add them again.  The count is exact; the loss sums are added in another order by
    the two kernels: rtol 1e-5, as in test_gpu_two_tier.py::
    test_cut_launch_under_the_hot_tier_keeps_its_statistics_without_sync_cut."""
    sums = []
    for path in ("sync_cut", "exchange"):
        e, ids = _engine(problem, bias=False)
        _hot_set(e, ids)
        hb, tot = (torch.zeros(H, D, device=e.Q.device) for _ in range(2))
        e.hot_tier_begin(hb)
        sc = torch.zeros(4, device=e.Q.device)
        _launch(e, ids, 0, scalars=sc, cut=True)
        if path == "sync_cut":
            e.sync_cut(hb, tot, False, None, None, None, 1.0, 0)
        else:
            e.hot_exchange(hb, tot, False, True)
        _launch(e, ids, 1)  # no scalars of its own: whatever it adds to sc is the first launch's, again
        e.hot_exchange(hb, tot, True, True)
        e.hot_tier_end()
        torch.cuda.synchronize()
        sums.append(sc.cpu().numpy())
        e.close()
    assert sums[0][3] == sums[1][3] == N
    assert np.allclose(sums[0], sums[1], rtol=1e-5, atol=0)


def test_tracking_skips_the_refill_of_the_wide_bias_while_it_is_clean(problem):
    """bias_wide_taken and bias_wide_synced: with tracking on, the launch after a launch works on the wide table it
    wrote back and does not read the dense vector again.  So a write the caller does NOT declare (bpr_bias_written)
    is overwritten by the next write-back, exactly as if it had not happened — that is the contract of
    bpr_set_bias_tracking, and the only way to see from outside that the refill was skipped."""
    out = []
    for undeclared in (True, False):
        e, ids = _engine(problem, bias=True)
        e.set_bias_tracking(True)
        _launch(e, ids, 0)
        if undeclared:
            e.item_bias.add_(1.0)
        _launch(e, ids, 1)
        torch.cuda.synchronize()
        out.append([t.cpu().numpy().copy() for t in (e.P, e.Q, e.item_bias)])
        e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_a_commit_makes_a_staled_partial_front_walkable_again(problem):
    """front_replaced: with partial snapshots, the lag-1 pipeline's cut overwrites the keys the partial front was
    sorted from (keys_front_stale: it can no longer be walked or completed); the commit that follows puts a new
    snapshot in front, and the next launch must be accepted."""
    e, ids = _engine(problem, bias=False, items=2048)
    e.set_tuning("partial_snapshot", 1)
    _launch(e, ids, 0, cut=True)
    e.adaptive_refresh_begin()
    e.adaptive_refresh_commit()
    assert e.snapshot_partial()
    _launch(e, ids, 1, cut=True)   # into the other key buffer
    e.adaptive_refresh_begin()
    _launch(e, ids, 2, cut=True)   # into the buffer the front was sorted from: the front is stale now
    with pytest.raises(Exception, match="partial snapshot"):
        _launch(e, ids, 0)
    e.adaptive_refresh_commit()
    _launch(e, ids, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(e.Q).all()
    e.close()
