"""bpr_train_stream_batched_scored — dynamic negatives and the WARP objective in the batched STREAM launch, under every
optimizer kind — against tests/vstream_scored_model.py (the mini-batch loop with scored draws; pinned on the CPU by
tests/test_vstream_scored_cpu.py) and against the stand-alone kernels bpr_sample_dynamic / bpr_sample_warp.

Tolerance of the sequential limit: the one tests/test_gpu_vstream.py (`agree`: 2e-5 relative to max(1, |w|), Adam and
RMSprop through close_mostly) and tests/test_gpu_adagrad.py (TOL = 2e-5, close) apply to the same kernel on given
negatives; the scalars to 2e-4 of their value, as test_gpu_vstream.py's loss.

The shapes: U = 40, I = 64, 200 triples; user U - 1 has seen all but one item and user U - 2 all but three (their
candidate lists are one item four times over, and three items with duplicates).  At I = 64 the 4,096 candidates of a
triple cannot all miss an unseen item, so the rank FALLBACK itself is reached in a case of its own, on
dynamic_cases.nearly_all_seen (I = 5,000; its seen rows are also longer than the staged list).
"""
import math

import numpy as np
import pytest

import dynamic_cases as dc
import vstream_scored_model as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, close_mostly, dev, make_engine, maxerr  # noqa: E402

U, I, N, REG, TOL = vm.U, vm.I, vm.N, vm.REG, vm.TOL
DYNAMIC, WARP = vm.DYNAMIC, vm.WARP
OFFSET = 1000


def agree(got, want, cfg, tol=TOL):
    """tests/test_gpu_vstream.py `agree` (Adagrad: tests/test_gpu_adagrad.py's close)."""
    if cfg["kind"] in (2, 3):
        return close_mostly(got, want, tol, cap=10 * cfg["lr"])
    return close(got, want, tol)


_problems = {}


def problem(d, bias, seed):
    """The tables, the seen CSR and the triples of one (d, bias, seed): computed once, never written to."""
    key = (d, bias, seed)
    if key not in _problems:
        P, Q, b, indptr, indices = vm.problem(U, I, d, bias, seed, vm.SCALE)
        users, pos = vm.triples(indptr, indices, N, seed + 100)
        for a in (P, Q, b, indptr, indices, users, pos):
            if a is not None:
                a.setflags(write=False)
        _problems[key] = (P, Q, b, indptr, indices, users, pos)
    return _problems[key]


def engine(pr, cfg, kind, K, margin=None, direct=-1):
    P, Q, b, indptr, indices, _, _ = pr
    e = make_engine(P.copy(), Q.copy(), None if b is None else b.copy(), REG)
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(**cfg)
    st = e.alloc_opt_state()
    if kind == DYNAMIC:
        e.set_dynamic(K)
    else:
        e.set_warp(K, vm.warp_margin(P.shape[1]) if margin is None else margin)
    e.set_tuning("vs_direct", direct)
    return e, st


def launch(e, users, pos, B, kind, seed, cuts, max_inflight=1):
    """One stream cut into len(cuts) + 1 calls at multiples of B; returns (neg, tries, scalars) as numpy."""
    n = len(users)
    u, p = dev(users), dev(pos)
    neg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    tries = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    edges = [0] + list(cuts) + [n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        e.train_stream_batched_scored(u[lo:hi], p[lo:hi], B, kind, neg=neg[lo:hi], tries=tries[lo:hi], seed=seed,
                                      offset=OFFSET + lo, max_inflight=max_inflight, scalars=sc)
    return neg.cpu().numpy(), tries.cpu().numpy(), sc.cpu().numpy().astype(np.float64)


def tables(e, st):
    out = {"P": e.P.cpu().numpy(), "Q": e.Q.cpu().numpy()}
    if e.item_bias is not None:
        out["b"] = e.item_bias.cpu().numpy()
    for k, t in st.items():
        if t is not None:
            out[k] = t.cpu().numpy()
    return out


# ---- 1. the symbol exists and runs; the old entry points keep refusing --------------------------------------------------
def test_the_entry_point_runs_and_the_old_ones_still_refuse():
    import ctypes

    from revisit_bpr import fast, native
    from test_gpu_warp import small_model

    pr = problem(32, True, 1)
    e, _ = engine(pr, vm.OPTS["adam_09"], DYNAMIC, 4)
    assert hasattr(e._lib, "bpr_train_stream_batched_scored")
    users, pos = pr[5], pr[6]
    P0 = e.P.clone()
    neg, tries, sc = launch(e, users, pos, 32, DYNAMIC, 3, ())
    e.flush_lazy()
    assert (neg > 0).all() and (tries == 1).all() and sc[3] == N and e.step_count == math.ceil(N / 32)
    assert not torch.equal(e.P, P0)
    lib, ctx = e._lib, e._ctx
    u, p = dev(users), dev(pos)
    out = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    before = (e.P.clone(), e.Q.clone(), e.step_count)
    for kind in (DYNAMIC, WARP):
        assert lib.bpr_train_stream_batched(ctx, u.data_ptr(), p.data_ptr(), out.data_ptr(), N, 32, kind,
                                            ctypes.c_float(0.1), 1, 0, 0, None) == native.ERR_UNSUPPORTED
        assert lib.bpr_train_strict(ctx, u.data_ptr(), p.data_ptr(), out.data_ptr(), N, 32, kind,
                                    ctypes.c_float(0.1), 1, 0, 0, None) == native.ERR_UNSUPPORTED
        assert lib.bpr_step(ctx, u.data_ptr(), p.data_ptr(), out.data_ptr(), N, native.MODE_STRICT, kind,
                            ctypes.c_float(0.1), 1, 0, None, None, None) == native.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -7).all() and torch.equal(e.P, before[0]) and torch.equal(e.Q, before[1])
    assert e.step_count == before[2]
    _, model, t = small_model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for cls in (fast.BatchedStreamTrainer, fast.StrictTrainer):
        with pytest.raises(ValueError, match="DynamicSampler"):
            cls(model, opt, t["users"], t["items"], t["indptr"], t["indices"], sampler="dynamic")
        with pytest.raises(ValueError, match="plain-SGD STREAM kernel only"):
            cls(model, opt, t["users"], t["items"], t["indptr"], t["indices"], sampler="warp")


# ---- 2. the first virtual batch is the stand-alone kernels' draw, element for element --------------------------------------
@pytest.mark.parametrize("d", [8, 32, 128, 256])
@pytest.mark.parametrize("bias", [False, True])
def test_first_batch_is_the_stand_alone_draw(d, bias):
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


@pytest.mark.parametrize("kind", [DYNAMIC, WARP])
def test_the_rank_fallback_and_a_user_with_nothing_unseen(kind):
    """dynamic_cases.nearly_all_seen: user 1 has seen all but item 1234 of 4,999 (about 0.8 of 4,096 candidates are
    accepted: "fewer than K" and "none: the rank pick" both occur over the 64 triples — the CPU files show it), user 2
    has seen everything (item 0, the pad item: no embedding gradient).  One virtual batch on flushed tables."""
    ed = dc.nearly_all_seen(d=32)
    n = len(ed["users"])
    users = ed["users"].copy()
    users[-8:] = 2
    pos = np.full(n, 7, np.int32)
    e = make_engine(ed["P"].copy(), ed["Q"].copy(), None, REG)
    e.bind_seen_csr(dev(ed["indptr"]), dev(ed["indices"]))
    e.set_optimizer(**vm.OPTS["adam_09"])
    e.alloc_opt_state()
    u, p = dev(users), dev(pos)
    if kind == DYNAMIC:
        e.set_dynamic(8)
        want_neg, want_tries = e.sample_dynamic(u, 8, seed=dc.SEED, offset=OFFSET).cpu().numpy(), np.ones(n, np.int32)
    else:
        e.set_warp(8, 1e6)  # everything violates: the first candidate, tries 1 — the fallback's pick included
        wn, wt = e.sample_warp(u, p, 8, seed=dc.SEED, offset=OFFSET, margin=1e6)
        want_neg, want_tries = wn.cpu().numpy(), wt.cpu().numpy()
    assert (want_neg[:-8] == ed["unseen"]).all() and not want_neg[-8:].any()
    neg, tries, sc = launch(e, users, pos, n, kind, dc.SEED, ())
    e.flush_lazy()
    assert np.array_equal(neg, want_neg) and np.array_equal(tries, want_tries) and sc[3] == n
    assert torch.isfinite(e.P).all() and torch.isfinite(e.Q).all() and not e.Q[0].any()


# ---- 3. the step, given the kernel's own picks ------------------------------------------------------------------------------
# (d, bias, optimizer, kind, K, B, vs_direct): every width, B, optimizer kind, K of both samplers, bias on and off,
# vs_direct 0 and 1 at B = 32 — each value of each, not their product
STEP_CASES = [
    (8, True, "sgd", DYNAMIC, 1, 32, 1), (8, False, "adam_09", WARP, 10, 4, -1), (8, True, "adagrad", WARP, 32, 1, -1),
    (32, False, "nesterov", DYNAMIC, 4, 32, 0), (32, True, "adam_09", DYNAMIC, 32, 32, 1),
    (32, True, "rmsprop", WARP, 1, 32, 1), (32, False, "adagrad", WARP, 10, 32, 0),
    (128, True, "adam_09", WARP, 10, 32, 0), (128, False, "sgd", WARP, 32, 4, -1),
    (128, True, "adagrad", DYNAMIC, 4, 32, 1), (128, False, "rmsprop", DYNAMIC, 32, 1, -1),
    (256, False, "adam_09", DYNAMIC, 4, 32, 1), (256, True, "nesterov", WARP, 10, 32, 1),
    (256, True, "rmsprop", DYNAMIC, 1, 4, -1), (256, False, "adagrad", WARP, 1, 32, 0),
    (256, True, "sgd", WARP, 32, 32, 0),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_sequential_limit_follows_the_model_fed_with_the_reported_picks(case):
    d, bias, opt, kind, K, B, direct = case
    cfg = vm.OPTS[opt]
    pr = problem(d, bias, 3)
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
    want = {"P": Pm, "Q": Qm, "b": bm}
    ms = res["state"]
    if cfg["kind"] in (1, 2) or cfg.get("momentum", 0) > 0:
        want.update(mP=ms["mP"], mQ=ms["mQ"], mb=ms.get("mb"))
    if cfg["kind"] in (2, 3, 4):
        want.update(vP=ms["vP"], vQ=ms["vQ"], vb=ms.get("vb"))
    for k, w in want.items():
        if w is None:
            continue
        print(f"{case} {k}: max err {maxerr(got[k], w):.3g}")
        assert agree(got[k], w, cfg), (k, maxerr(got[k], w))
    assert np.abs(Pm - P).max() > 1e-3 and np.abs(Qm - Q).max() > 1e-3  # the tables really moved
    assert not got["P"][0].any() and not got["Q"][0].any()
    stepped = int((neg >= 0).sum())
    print(f"{case}: {N - stepped} skipped, scalars {sc} model {res['scalars']}")
    assert sc[3] == stepped == res["scalars"][3]
    for k in range(3):
        assert abs(sc[k] - res["scalars"][k]) <= 2e-4 * abs(res["scalars"][k]), (k, sc[k], res["scalars"][k])
    # rows no STEPPED triple touches — those that skipped triples alone touch among them — are the zero-gradient
    # replay's: the model's, above; where that replay moves nothing (SGD, Adagrad), the start's bits
    if cfg["kind"] in (0, 4):
        for k, n_rows, rows, start in (("P", U, res["rows"][0], P), ("Q", I, res["rows"][1], Q)):
            rest = np.setdiff1d(np.arange(n_rows), sorted(rows))
            assert np.array_equal(got[k][rest].view(np.int32), start[rest].view(np.int32)), k
    if kind == WARP and K > 1:
        only_skipped = set(users[neg < 0].tolist()) - set(users[neg >= 0].tolist())
        print(f"{case}: users that only skipped triples touch: {sorted(only_skipped)}")


# ---- 4. later batches' picks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vm.PICK_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_later_batches_draw_on_the_views_the_model_draws_on(case):
    """The model draws every triple from its own tables — which follow the device's reported picks, so they stay
    within the sequential limit's tolerance of the device's — and a triple may disagree only where the model's deciding
    gap is below the bound that tolerance gives (vstream_scored_model.gap_bound); at most CAP of the triples."""
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


# ---- 5. the chip full: properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,kind,K", [("adam_09", WARP, 10), ("adagrad", DYNAMIC, 4), ("rmsprop", WARP, 32)])
def test_full_chip_properties(opt, kind, K):
    from revisit_bpr.datasets import synthetic

    data = synthetic.generate(2000, 500, 20000, median_per_user=10, seed=6)
    d, Bv, n = 64, 256, data.nnz
    rng = np.random.default_rng(9)
    P = ((rng.random((data.num_users, d)) - 0.5)).astype(np.float32)
    Q = ((rng.random((data.num_items, d)) - 0.5)).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b = np.zeros(data.num_items, np.float32)
    e = make_engine(P, Q, b, REG)
    e.bind_seen_csr(dev(data.indptr), dev(data.indices))
    e.set_optimizer(**vm.OPTS[opt])
    st = e.alloc_opt_state()
    if kind == DYNAMIC:
        e.set_dynamic(K)
    else:
        e.set_warp(K, 1.0)
    pu, pi = e.shuffle_epoch(dev(data.users), dev(data.items), seed=5)
    neg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    tries = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    e.train_stream_batched_scored(pu, pi, Bv, kind, neg=neg, tries=tries, seed=3, offset=OFFSET, max_inflight=0,
                                  scalars=sc)
    e.flush_lazy()
    torch.cuda.synchronize()
    assert e.step_count == math.ceil(n / Bv)
    for k, t in list(st.items()) + [("P", e.P), ("Q", e.Q), ("b", e.item_bias)]:
        if t is not None:
            assert bool(torch.isfinite(t).all()), k
    neg, tries, users = neg.cpu().numpy(), tries.cpu().numpy(), pu.cpu().numpy()
    assert ((neg > 0) | (neg == -1)).all() and ((neg < 0) == (tries == 0)).all()
    assert (tries[neg > 0] >= 1).all() and (tries <= K).all()
    if kind == DYNAMIC:
        assert (tries == 1).all()
    seen = {u: set(data.indices[data.indptr[u]:data.indptr[u + 1]].tolist()) for u in np.unique(users).tolist()}
    assert all(j < 0 or j not in seen[u] for u, j in zip(users.tolist(), neg.tolist()))
    assert int(sc[3]) == int((neg >= 0).sum()) > 0
    before = [t.clone() for t in (e.P, e.Q, e.item_bias)]
    e.flush_lazy()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(before, (e.P, e.Q, e.item_bias)))
    assert not e.P[0].any() and not e.Q[0].any()


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,sampler", [("adagrad", "warp"), ("adam", "dynamic")])
def test_scored_batched_stream_trainer_trains_two_epochs(opt, sampler):
    from revisit_bpr import fast
    from test_gpu_warp import small_model

    data, model, t = small_model()
    optimizer = (torch.optim.Adagrad(model.parameters(), lr=0.05) if opt == "adagrad"
                 else torch.optim.Adam(model.parameters(), lr=0.01, betas=(0.1, 0.999)))
    tr = fast.ScoredBatchedStreamTrainer(model, optimizer, t["users"], t["items"], t["indptr"], t["indices"],
                                         sampler=sampler, candidates=4, max_sampled=10, margin=1.0, batch_size=64, seed=5)
    before = model.logits_model.get_features()["user"].data.clone()
    first, second = tr.train_epoch(), tr.train_epoch()
    model.sync()
    for stats in (first, second):
        assert np.isfinite(stats["loss"]) and np.isfinite(stats["bpr_loss"]) and stats["bpr_loss"] > 0
        if sampler == "warp":
            assert 0 < stats["triples"] <= data.nnz
        else:
            assert stats["triples"] == data.nnz
    after = model.logits_model.get_features()["user"].data
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    assert tr.engine.step_count == 2 * sum(math.ceil((min(lo + tr.chunk, tr.n) - lo) / 64)
                                           for lo in range(0, tr.n, tr.chunk))
    with pytest.raises(ValueError, match="dynamic.*warp"):
        fast.ScoredBatchedStreamTrainer(model, optimizer, t["users"], t["items"], t["indptr"], t["indices"],
                                        sampler="uniform")


# ---- 7. refusals of the new entry point -----------------------------------------------------------------------------------
def test_refusals_return_invalid_and_leave_the_tables_alone():
    from revisit_bpr import native

    pr = problem(32, True, 4)
    P, Q, b, indptr, indices, users, pos = pr
    e, st = engine(pr, vm.OPTS["adam_09"], DYNAMIC, 4)
    lib, ctx = e._lib, e._ctx
    u, p = dev(users), dev(pos)
    out = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    tensors = [e.P, e.Q, e.item_bias] + [t for t in st.values() if t is not None]
    before = [t.clone() for t in tensors]

    def call(c=ctx, uu=u.data_ptr(), pp=p.data_ptr(), kind=DYNAMIC, B=32):
        return lib.bpr_train_stream_batched_scored(c, uu, pp, out.data_ptr(), out.data_ptr(), N, B, kind, 1, 0, 1, None)

    def untouched():
        torch.cuda.synchronize()
        return (out == -7).all() and e.step_count == 0 and \
            all(torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(before, tensors))

    for kind in (0, 1, 2, 5, -1):  # given, uniform, adaptive, unknown
        assert call(kind=kind) == native.ERR_INVALID and untouched()
    assert call(uu=None) == native.ERR_INVALID and untouched()
    assert call(pp=None) == native.ERR_INVALID and untouched()
    assert call(B=0) == native.ERR_INVALID and untouched()
    assert call(c=None) == native.ERR_INVALID
    with pytest.raises(native.BprError) as ei:
        e.train_stream_batched_scored(u, p, 32, 1)
    assert ei.value.code == native.ERR_INVALID and untouched()
    # pending STRICT gradients
    j = dev(np.where(pos == 1, 2, 1).astype(np.int32))
    e.forward_grad(u[:32], p[:32], j[:32])
    assert call() == native.ERR_INVALID and b"pending" in lib.bpr_last_error() and untouched()
    # no seen CSR
    e2 = make_engine(P.copy(), Q.copy(), b.copy(), REG)
    e2.set_optimizer(**vm.OPTS["adam_09"])
    e2.alloc_opt_state()
    P2 = e2.P.clone()
    rc = e2._lib.bpr_train_stream_batched_scored(e2._ctx, u.data_ptr(), p.data_ptr(), out.data_ptr(), out.data_ptr(), N,
                                                 32, WARP, 1, 0, 1, None)
    torch.cuda.synchronize()
    assert rc == native.ERR_INVALID and b"seen CSR" in e2._lib.bpr_last_error()
    assert torch.equal(e2.P, P2) and (out == -7).all() and e2.step_count == 0
