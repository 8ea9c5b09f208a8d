"""The batched STREAM launch — bpr_train_stream_batched (given and uniform negatives) and bpr_train_stream_batched_scored
(dynamic negatives, WARP) — against its models at all six row layouts (G, E) of csrc/bpr_group_shape.h, with the 64-thread
block of the sequential limit and the 256-thread block of full concurrency.

The widths are vstream_scored_model.WIDTHS: per layout the smallest, the largest and a ragged width, where
tests/test_gpu_vstream_scored.py (d = 8, 32, 128, 256) and tests/test_gpu_vstream.py do not already run them; (64, 8) and
(64, 16), d = 257 .. 1024, are run by no other model comparison of the scored kinds.  The models, the tolerance
(vstream_scored_model.TOL through `agree`; scalars to 2e-4 of their value) and the helpers are those files'; the cases
are vstream_scored_model.WIDTH_STEP_CASES / WIDTH_PICK_CASES / WIDTH_FULL_CASES, which tests/test_vstream_widths_cpu.py
shows fit for purpose without a GPU (the caps have slack, skipped and late WARP triples occur, every case moves the last
column of a row, a dropped tail and a view one step off fail the assertions made here).

The shapes: U = 40, I = 64, 200 triples, as in tests/test_gpu_vstream_scored.py.
"""
import math

import numpy as np
import pytest

import oracle
import vstream_scored_model as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import dev, make_engine, maxerr  # noqa: E402
from test_gpu_vstream import distinct_neg  # noqa: E402
from test_gpu_vstream_scored import OFFSET, agree, engine, launch, problem, tables  # noqa: E402

U, I, N, REG, TOL = vm.U, vm.I, vm.N, vm.REG, vm.TOL
DYNAMIC, WARP, UNIFORM = vm.DYNAMIC, vm.WARP, vm.UNIFORM
ident = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def compare(what, got, want, cfg):
    """Every tensor of `want` against the engine's, max error printed, at TOL through `agree`."""
    for k, w in want.items():
        if w is None:
            continue
        print(f"{what} {k}: max err {maxerr(got[k], w):.3g}")
        assert agree(got[k], w, cfg), (k, maxerr(got[k], w))


def untouched_rows_keep_their_bits(got, rows, start, cfg):
    """SGD and Adagrad move nothing on a zero gradient: rows no stepped triple touches are the start's, bit for bit."""
    if cfg["kind"] not in (0, 4):
        return
    for k, touched, w0 in (("P", rows[0], start[0]), ("Q", rows[1], start[1])):
        rest = np.setdiff1d(np.arange(len(w0)), sorted(touched))
        assert rest.size and np.array_equal(got[k][rest].view(np.int32), w0[rest].view(np.int32)), k


# ---- a. scored kinds: the first virtual batch is the stand-alone kernels' draw, element for element ------------------------
@pytest.mark.parametrize("d", vm.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
def test_first_batch_is_the_stand_alone_draw(d, bias):
    """tests/test_gpu_vstream_scored.py's test of the same name at the new widths.  bpr_sample_dynamic and
    bpr_sample_warp are themselves held to the numpy models at sixteen entries a lane (tests/test_gpu_dynamic.py,
    tests/test_gpu_warp.py): a model comparison at one remove."""
    pr = problem(d, bias, 2)
    users, pos = pr[5], pr[6]
    B = 32
    for kind, Ks in ((DYNAMIC, (1, 4, 32)), (WARP, (1, 10, 32))):
        for K in Ks:
            e, _ = engine(pr, vm.OPTS["adam_09"], kind, K)
            u, p = dev(users[:B]), dev(pos[:B])
            if kind == DYNAMIC:
                want_neg = e.sample_dynamic(u, K, seed=5, offset=OFFSET).cpu().numpy()
                want_tries = np.ones(B, np.int32)
            else:
                wn, wt = e.sample_warp(u, p, K, seed=5, offset=OFFSET, margin=vm.warp_margin(d))
                want_neg, want_tries = wn.cpu().numpy(), wt.cpu().numpy()
            neg, tries, _ = launch(e, users[:3 * B], pos[:3 * B], B, kind, 5, ())
            assert np.array_equal(neg[:B], want_neg), (kind, K, np.flatnonzero(neg[:B] != want_neg))
            assert np.array_equal(tries[:B], want_tries), (kind, K)
            if kind == WARP:  # skipped triples and late violators both occur
                assert (want_neg < 0).any() if K == 1 else (want_tries > 1).any()


# ---- b. scored kinds: the sequential limit, given the reported picks ------------------------------------------------------
@pytest.mark.parametrize("case", vm.WIDTH_STEP_CASES, ids=ident)
def test_sequential_limit_follows_the_model_fed_with_the_reported_picks(case):
    d, bias, opt, kind, K, B, direct = case
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, vm.STEP_SEED)
    P, Q, b, indptr, indices, users, pos = pr
    e, st = engine(pr, cfg, kind, K, direct=direct)
    cut = (N // 2 // B) * B  # one launch cut into two calls: the step counter and the Philox counter carry on
    neg, tries, sc = launch(e, users, pos, B, kind, 7, (cut,))
    e.flush_lazy()
    assert e.step_count == math.ceil(N / B)
    assert ((neg < 0) == (tries == 0)).all() and (tries <= K).all() and (neg != 0).all()
    if kind == DYNAMIC:
        assert (tries == 1).all()
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    res = vm.run(Pm, Qm, bm, indptr, indices, users, pos, B, kind, K, vm.warp_margin(d), cfg, REG, seed=7, offset=OFFSET,
                 given=(neg, tries), tol=TOL)
    got = tables(e, st)
    compare(case, got, dict({"P": Pm, "Q": Qm, "b": bm}, **vm.want_state(cfg, res["state"])), cfg)
    assert np.abs(Pm - P).max() > 1e-3 and np.abs(Qm - Q).max() > 1e-3  # the tables really moved
    assert not got["P"][0].any() and not got["Q"][0].any()
    stepped = int((neg >= 0).sum())
    print(f"{case}: {N - stepped} skipped, scalars {sc} model {res['scalars']}")
    assert sc[3] == stepped == res["scalars"][3]
    for k in range(3):
        assert abs(sc[k] - res["scalars"][k]) <= 2e-4 * abs(res["scalars"][k]), (k, sc[k], res["scalars"][k])
    untouched_rows_keep_their_bits(got, res["rows"], (P, Q), cfg)


# ---- c. scored kinds: later batches' picks -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vm.WIDTH_PICK_CASES, ids=ident)
def test_later_batches_draw_on_the_views_the_model_draws_on(case):
    """tests/test_gpu_vstream_scored.py's test of the same name on WIDTH_PICK_CASES: a triple may disagree with the
    model (which follows the device's reported picks) only where the model's deciding gap is below
    vstream_scored_model.gap_bound, and on at most CAP of the triples."""
    d, bias, opt, kind, K, B, seed = case
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, seed)
    P, Q, b, indptr, indices, users, pos = pr
    e, _ = engine(pr, cfg, kind, K)
    cut = (N // 2 // B) * B
    neg, tries, _ = launch(e, users, pos, B, kind, seed, (cut,))
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    res = vm.run(Pm, Qm, bm, indptr, indices, users, pos, B, kind, K, vm.warp_margin(d), cfg, REG, seed=seed,
                 offset=OFFSET, given=(neg, tries), tol=TOL)
    differ, unexcused = vm.excused(neg, tries, res)
    print(f"{case}: {differ} of {N} differ, {unexcused} outside the bound; later batches: "
          f"{int(((neg != res['neg']) | (tries != res['tries']))[B:].sum())}")
    assert unexcused == 0 and differ <= vm.CAP * N
    assert len(set(neg[B:].tolist())) > 10  # the later batches do draw


# ---- d. given and uniform negatives: the sequential limit ------------------------------------------------------------------
# (d, bias, optimizer): every (layout, optimizer kind) pair of the five layouts tests/test_gpu_vstream.py's own
# sequential-limit test (d = 32, 50, 128, 256) leaves out or runs without Adagrad and without comparing the state
GIVEN_CASES = [
    (33, True, "sgd"), (33, False, "adam_09"), (33, True, "adagrad"), (64, False, "nesterov"), (64, True, "rmsprop"),
    (65, False, "sgd"), (65, True, "nesterov"), (65, True, "adam_09"), (65, False, "rmsprop"), (65, False, "adagrad"),
    (129, True, "sgd"), (129, False, "nesterov"), (129, False, "adam_09"), (129, True, "rmsprop"), (129, True, "adagrad"),
    (257, False, "sgd"), (257, True, "rmsprop"), (500, True, "adam_09"), (500, False, "adagrad"), (512, True, "nesterov"),
    (512, False, "adam_09"),
    (513, True, "adam_09"), (513, False, "nesterov"), (1000, True, "adagrad"), (1000, False, "sgd"),
    (1024, True, "rmsprop"), (1024, False, "adam_09"),
]


def given_triples(pr, seed):
    """The 200 triples of the problem with negatives of the caller's: users, positives and a negative repeated inside
    the first batch, a pad user and a pad item (their embedding gradients are dropped)."""
    users, pos = pr[5].copy(), pr[6].copy()
    neg = np.random.default_rng(seed).integers(1, I, N).astype(np.int32)
    users[:4] = users[4]
    pos[6:10] = pos[10]
    neg[12:15] = pos[10]
    users[17], pos[18] = 0, 0
    return users, pos, distinct_neg(pos, neg, I)


@pytest.mark.parametrize("case", GIVEN_CASES, ids=ident)
def test_given_negatives_sequential_limit_tables_and_state(case):
    d, bias, opt = case
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, 5)
    P, Q, b = pr[0], pr[1], pr[2]
    users, pos, neg = given_triples(pr, d)
    B = 24  # 200 = 8 * 24 + 8: a ragged last batch
    e = make_engine(P.copy(), Q.copy(), None if b is None else b.copy(), REG)
    e.set_optimizer(**cfg)
    st = e.alloc_opt_state()
    sc = torch.zeros(4, device="cuda")
    cut = 4 * B  # two launches: pending steps and the step counter carry across
    for sl in (slice(0, cut), slice(cut, N)):
        e.train_stream_batched(dev(users[sl]), dev(pos[sl]), B, sampler=0, neg=dev(neg[sl]), max_inflight=1, scalars=sc)
    e.flush_lazy()
    assert e.step_count == math.ceil(N / B) and int(sc[3]) == N
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    ms, rows = vm.given_loop(Pm, Qm, bm, users, pos, neg, B, cfg, REG)
    got = tables(e, st)
    compare(case, got, dict({"P": Pm, "Q": Qm, "b": bm}, **vm.want_state(cfg, ms)), cfg)
    assert np.abs(Pm[:, d - 1] - P[:, d - 1]).max() > 50 * TOL and np.abs(Qm[:, d - 1] - Q[:, d - 1]).max() > 50 * TOL
    assert not got["P"][0].any() and not got["Q"][0].any()
    untouched_rows_keep_their_bits(got, rows, (P, Q), cfg)


@pytest.mark.parametrize("d,bias,opt", [(257, True, "adam_09"), (1000, False, "adagrad")])
def test_uniform_negatives_sequential_limit_on_the_staged_list(d, bias, opt):
    """sampler = 1 at the two layouts no test of the uniform kind runs in the sequential limit: the seen lists staged in
    LDS beside rows of 3 * G * E words; the picks are oracle.sample_uniform's, the tables vm.uniform_loop's."""
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, 6)
    P, Q, b, indptr, indices, users, pos = pr
    B = 24
    e = make_engine(P.copy(), Q.copy(), None if b is None else b.copy(), REG)
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(**cfg)
    st = e.alloc_opt_state()
    neg = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    cut = 4 * B
    for lo, hi in ((0, cut), (cut, N)):
        e.train_stream_batched(dev(users[lo:hi]), dev(pos[lo:hi]), B, sampler=1, neg=neg[lo:hi], seed=9,
                               offset=OFFSET + lo, max_inflight=1)
    e.flush_lazy()
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    want_neg, ms = vm.uniform_loop(Pm, Qm, bm, indptr, indices, users, pos, B, cfg, REG, seed=9, offset=OFFSET)
    assert np.array_equal(neg.cpu().numpy(), want_neg)
    compare((d, bias, opt, "uniform"), tables(e, st), dict({"P": Pm, "Q": Qm, "b": bm}, **vm.want_state(cfg, ms)), cfg)


# ---- e. the 256-thread block and its LDS -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vm.WIDTH_FULL_CASES, ids=ident)
def test_full_concurrency_one_virtual_batch_is_the_stand_alone_draw_and_one_step(case):
    """max_inflight = 0: blocks of 256 threads, 4 groups (G = 64) or 8 (G = 32), each with a staged seen list of 512
    words and three rows of G * E — 57,344 B of dynamic LDS at (64, 16), the launch's largest.  With B >= n the launch
    is ONE virtual batch on flushed tables: every view is the starting table, so the picks and tries of the whole
    launch are the stand-alone kernels' (the uniform kind's: oracle.sample_uniform's) bit for bit, and every row takes
    one optimizer step on its summed gradient — the model's single-batch step at TOL (fp32 atomics sum the five or so
    gradients of a row in any order).  A second flush_lazy changes no bit."""
    d, bias, opt, sampler, K, seed = case
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, seed)
    P, Q, b, indptr, indices, users, pos = pr
    B = 256
    u, p = dev(users), dev(pos)
    if sampler == UNIFORM:
        e = make_engine(P.copy(), Q.copy(), None if b is None else b.copy(), REG)
        e.bind_seen_csr(dev(indptr), dev(indices))
        e.set_optimizer(**cfg)
        st = e.alloc_opt_state()
        out = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        sc = torch.zeros(4, device="cuda")
        e.train_stream_batched(u, p, B, sampler=1, neg=out, seed=seed, offset=OFFSET, max_inflight=0, scalars=sc)
        neg, tries, sc = out.cpu().numpy(), np.ones(N, np.int32), sc.cpu().numpy().astype(np.float64)
        want_neg = oracle.sample_uniform(indptr, indices, I, users, seed, OFFSET)
        want_tries = tries
    else:
        e, st = engine(pr, cfg, sampler, K)
        if sampler == DYNAMIC:
            want_neg, want_tries = e.sample_dynamic(u, K, seed=seed, offset=OFFSET).cpu().numpy(), np.ones(N, np.int32)
        else:
            wn, wt = e.sample_warp(u, p, K, seed=seed, offset=OFFSET, margin=vm.warp_margin(d))
            want_neg, want_tries = wn.cpu().numpy(), wt.cpu().numpy()
        neg, tries, sc = launch(e, users, pos, B, sampler, seed, (), max_inflight=0)
    assert np.array_equal(neg, want_neg), np.flatnonzero(neg != want_neg)
    assert np.array_equal(tries, want_tries)
    if sampler == WARP:
        assert (neg < 0).any() and (K == 1 or (tries > 1).any())
    e.flush_lazy()
    assert e.step_count == 1 and sc[3] == (neg >= 0).sum()
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    if sampler == UNIFORM:
        ms, rows = vm.given_loop(Pm, Qm, bm, users, pos, neg, B, cfg, REG)
    else:
        res = vm.run(Pm, Qm, bm, indptr, indices, users, pos, B, sampler, K, vm.warp_margin(d), cfg, REG, seed=seed,
                     offset=OFFSET, given=(neg, tries))
        ms, rows = res["state"], res["rows"]
        for k in range(3):
            assert abs(sc[k] - res["scalars"][k]) <= 2e-4 * abs(res["scalars"][k]), (k, sc[k], res["scalars"][k])
    got = tables(e, st)
    compare(case, got, dict({"P": Pm, "Q": Qm, "b": bm}, **vm.want_state(cfg, ms)), cfg)
    assert np.abs(Pm[:, d - 1] - P[:, d - 1]).max() > 50 * TOL and np.abs(Qm[:, d - 1] - Q[:, d - 1]).max() > 50 * TOL
    assert not got["P"][0].any() and not got["Q"][0].any()
    untouched_rows_keep_their_bits(got, rows, (P, Q), cfg)
    tensors = [e.P, e.Q] + [t for t in (e.item_bias,) + tuple(st.values()) if t is not None]
    before = [t.clone() for t in tensors]
    e.flush_lazy()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(before, tensors))


@pytest.mark.parametrize("opt,kind,K", [("adam_09", WARP, 10), ("adagrad", DYNAMIC, 4)])
def test_full_concurrency_two_virtual_batches_at_1024_properties(opt, kind, K):
    """Two virtual batches in flight in blocks of 256 threads at (64, 16): staleness makes the bits run-dependent, so
    only what tests/test_gpu_vstream_scored.py's full-chip test asserts — the count is conserved, everything is finite,
    no pick is a seen item, a second flush changes nothing."""
    d = 1024
    pr = problem(d, True, 8)
    P, Q, b, indptr, indices, users, pos = pr
    e, st = engine(pr, vm.OPTS[opt], kind, K)
    neg, tries, sc = launch(e, users, pos, N // 2, kind, 3, (), max_inflight=0)
    e.flush_lazy()
    torch.cuda.synchronize()
    assert e.step_count == 2
    tensors = {k: t for k, t in list(st.items()) + [("P", e.P), ("Q", e.Q), ("b", e.item_bias)] if t is not None}
    for k, t in tensors.items():
        assert bool(torch.isfinite(t).all()), k
    assert ((neg > 0) | (neg == -1)).all() and ((neg < 0) == (tries == 0)).all()
    assert (tries[neg > 0] >= 1).all() and (tries <= K).all()
    if kind == DYNAMIC:
        assert (tries == 1).all()
    seen = {u: set(indices[indptr[u]:indptr[u + 1]].tolist()) for u in np.unique(users).tolist()}
    assert all(j < 0 or j not in seen[u] for u, j in zip(users.tolist(), neg.tolist()))
    assert int(sc[3]) == int((neg >= 0).sum()) > 0
    before = {k: t.clone() for k, t in tensors.items()}
    e.flush_lazy()
    torch.cuda.synchronize()
    assert all(torch.equal(before[k].view(torch.int32), t.view(torch.int32)) for k, t in tensors.items())
    assert not e.P[0].any() and not e.Q[0].any() and not torch.equal(e.P, dev(P))
