"""The LDS tier of k_stream's hot block (r6: `bpr_set_hot_lds`, csrc/bpr_hotlds.hip) against the CPU oracle and
against the plain kernel.

What the tier may change is WHEN a workgroup sees the other workgroups' updates of the hottest rows (one launch
late); what it may not change:
  * with one group in flight it is exactly sequential SGD (the oracle's `train_stream_seq`), sampler included;
  * nothing is lost or counted twice: the launch's deltas are the exact sums (first-order test on a zero table);
  * sampled negatives are valid at full concurrency (never the pad item, never a seen one; uniform picks are
    the plain kernel's);
  * the fused cut after the launch sees the table with every workgroup's flush folded in;
  * item_bias, loss statistics and the pad rows behave as in the plain kernel.
The G = 32 instantiations (d <= 128, the one bench.py times among them) are held to the oracle triple by triple
twice: with one group in flight, and with both groups of a wave at work on a stream whose two halves never share a
row (hotlds_model.two_half_stream) — the timed configuration, where the groups share the LDS delta block.
"""
import numpy as np
import pytest

import hotlds_model
import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr, rand_problem  # noqa: E402


def skewed_problem(U, I, d, n, seed, max_seen=40):
    rng = np.random.default_rng(seed)
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    lens = rng.integers(1, max_seen, U)
    lens[0] = 0
    rows = [np.sort(rng.choice(np.arange(1, I), size=int(k), replace=False)).astype(np.int32) for k in lens]
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    users = rng.integers(1, U, n).astype(np.int32)
    pos = (1 + (rng.zipf(1.3, n) % (I - 1))).astype(np.int32)  # a few rows take most of the positives
    return P, Q, indptr, np.concatenate(rows), users, pos, rng


@pytest.mark.parametrize("seen", ["", "list"])
@pytest.mark.parametrize("d,run_len,sampler,bias", [(256, 8, 1, False), (256, 3, 2, False), (512, 5, 0, True),
                                                     (1024, 8, 2, True)])
def test_lds_tier_sequential_equals_b1_sgd(d, run_len, sampler, bias, seen, monkeypatch):
    """(seen = "list": the groups' staged sorted seen lists beside the rows instead of the I-bit bitmaps — what the
    tier takes by itself for item tables too large for bitmaps.)
    One group in flight (G = 64: a whole wave) == the oracle's sequential SGD in planned order, three launches
    in a row (flush -> fold -> next launch reads the folded table), with 5 of the 12 hot rows in LDS and the other
    7 in the global block."""
    if seen:
        if sampler == 0:
            pytest.skip("given negatives: no seen structure")
        monkeypatch.setenv("BPR_SEEN", seen)
    P, Q, indptr, indices, users, pos, rng = skewed_problem(120, 80, d, 1400, d + run_len)
    b = (rng.normal(0, 0.1, Q.shape[0]).astype(np.float32)) if bias else None
    reg = (0.01, 0.02, 0.03)
    e = make_engine(P, Q, b, reg)
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(kind=0, lr=0.05)
    e.set_stream_opts(True, run_len)
    e.set_hot_rows(12, 1)
    e.set_hot_lds(8, always=True)  # (asks for 8 ...)
    pu, pp = e.plan_epoch(dev(users), dev(pos), chunk=len(users), seed=3)
    Po, Qo, bo = P.copy(), Q.copy(), None if b is None else b.copy()
    upl, ppl = pu.cpu().numpy(), pp.cpu().numpy()
    given = rng.integers(1, Q.shape[0], len(users)).astype(np.int32)
    sco = np.zeros(4)
    sc = torch.zeros(4, device="cuda")
    for launch in range(3):
        if sampler == 2:
            e.adaptive_refresh()
            QT, sigma = oracle.adaptive_stats(Qo)
            snap = dict(order=oracle.adaptive_order(QT), sigma=sigma, adaptive_p=0.05)
        else:
            snap = {}
        negs = dev(given) if sampler == 0 else torch.zeros_like(pu)
        e.train_stream(pu, pp, sampler=sampler, neg=negs, adaptive_p=0.05, seed=11, offset=launch * len(users),
                       max_inflight=1, scalars=sc)
        assert e.stream_lds_rows() == 8
        neg_o = given.copy() if sampler == 0 else np.zeros(len(users), np.int32)
        sco += oracle.train_stream_seq(Po, Qo, bo, upl, ppl, neg_o, sampler, 0.05, reg, indptr=indptr,
                                       indices=indices, seed=11, offset=launch * len(users), **snap)
        if sampler != 0:
            assert np.array_equal(negs.cpu().numpy(), neg_o), launch
        assert close(e.Q.cpu().numpy(), Qo, 1e-5), (launch, maxerr(e.Q.cpu().numpy(), Qo))
    assert close(e.P.cpu().numpy(), Po, 1e-5), maxerr(e.P.cpu().numpy(), Po)
    if bias:
        assert close(e.item_bias.cpu().numpy(), bo, 1e-5)
    assert close(sc.cpu().numpy()[:3], sco[:3], 1e-4) and int(sc[3]) == 3 * len(users)


@pytest.mark.parametrize("hot_rows,replicas,lds", [(16, 1, 8), (50, 4, 50), (50, 1, 20)])
def test_lds_tier_loses_nothing_under_chip_wide_contention(hot_rows, replicas, lds):
    """100k triples on 50 item rows from every CU at once, part of the rows in LDS: on a zero item table with a
    tiny learning rate every triple contributes lr x (gradient at the initial point) to first order, so the
    table after the launch is the exact sum — whatever a workgroup saw of the others meanwhile."""
    U, I, d, n = 20000, 60, 128, 100_000
    rng = np.random.default_rng(0)
    P = ((rng.random((U, d)) - 0.5) * 0.2).astype(np.float32)
    P[0] = 0
    Q0 = np.zeros((I, d), np.float32)
    users = rng.integers(1, U, size=n).astype(np.int32)
    pos = rng.integers(1, 51, size=n).astype(np.int32)
    neg = rng.integers(1, 51, size=n).astype(np.int32)
    lr = 1e-4
    e = make_engine(P, Q0, None, (0.0, 0.0, 0.0))
    e.set_optimizer(kind=0, lr=lr)
    e.set_hot_rows(hot_rows, replicas)
    e.set_hot_lds(lds, always=True)
    e.set_stream_opts(True, 8)
    pu, pi = e.plan_epoch(dev(users), dev(pos), n, seed=3)
    back = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(users, pos))}
    ng = np.asarray([neg[back[(int(a), int(b))]] for a, b in zip(pu.cpu().numpy(), pi.cpu().numpy())], np.int32)
    sc = torch.zeros(4, device="cuda")
    e.train_stream(pu, pi, sampler=0, neg=dev(ng), scalars=sc)
    assert e.stream_lds_rows() == min(lds, hot_rows)
    _, g, _ = oracle.dense_grad(P, Q0, None, pu.cpu().numpy(), pi.cpu().numpy(), ng, (0.0, 0.0, 0.0))
    dQ = e.Q.cpu().numpy().astype(np.float64) / -lr
    s0 = np.abs(g).max()
    assert s0 > 3 and np.abs(dQ - g).max() < 0.005 * s0, np.abs(dQ - g).max() / s0
    assert int(sc[3]) == n


@pytest.mark.parametrize("d,sampler,n,cut", [(128, 2, 120_000, True), (128, 1, 60_000, True), (64, 2, 90_000, True),
                                              (256, 2, 40_000, True), (32, 0, 50_000, True), (128, 2, 120_000, "async"),
                                              (64, 1, 70_000, "async")])
def test_lds_tier_cut_at_full_concurrency_sees_the_final_table(d, sampler, n, cut):
    """(cut = "async": the transpose on the side stream, the fold on the launch stream — with nothing running beside
    it here, the same exact snapshot.)
    The fused cut behind an LDS-tier launch: the snapshot committed afterwards is the oracle's order of the
    item table as the launch left it — every workgroup's flush folded in — launch after launch; the statistics
    count every triple; sampled negatives are valid (uniform: the plain kernel's picks triple by triple; adaptive
    picks read the live user rows, which at lr 0.05 and 20 triples per user have moved apart within the launch)."""
    P, Q, indptr, indices, users, pos, rng = skewed_problem(6000, 3000, d, n, d + n)
    engines = []
    for lds in (0, 64):
        e = make_engine(P, Q, None, (0.01, 0.02, 0.03))
        e.bind_seen_csr(dev(indptr), dev(indices))
        e.set_optimizer(kind=0, lr=0.05)
        e.set_stream_opts(True, 0)
        e.set_hot_lds(lds, always=True)
        engines.append(e)
    e0, e = engines
    pu, pi = e.plan_epoch(dev(users), dev(pos), n, seed=3)
    pu0, pi0 = e0.plan_epoch(dev(users), dev(pos), n, seed=3)
    assert torch.equal(pu, pu0) and torch.equal(pi, pi0)
    given = dev(rng.integers(1, Q.shape[0], n).astype(np.int32))
    sc = torch.zeros(4, device="cuda")
    e.adaptive_refresh()
    e0.adaptive_refresh()
    for launch in range(3):
        neg = given if sampler == 0 else torch.zeros_like(pu)
        e.train_stream(pu, pi, sampler=sampler, neg=neg, adaptive_p=0.05, seed=5, offset=launch * n, scalars=sc,
                       cut=cut)
        assert e.stream_lds_rows() > 0
        if launch == 0 and sampler != 0:
            neg0 = torch.zeros_like(pu)
            e0.train_stream(pu0, pi0, sampler=sampler, neg=neg0, adaptive_p=0.05, seed=5, offset=0)
            assert e0.stream_lds_rows() == 0
            if sampler == 1:  # uniform picks do not depend on the model: the same, triple by triple
                assert torch.equal(neg, neg0)
            un, nn = pu.cpu().numpy(), neg.cpu().numpy()
            for t in range(0, n, 211):
                assert nn[t] != 0 and nn[t] not in indices[indptr[un[t]]:indptr[un[t] + 1]]
        Qnow = e.Q.cpu().numpy()
        e.adaptive_refresh_begin()
        e.adaptive_refresh_commit()
        QT, sig = oracle.adaptive_stats(Qnow)
        got_o, got_s = e.adaptive_snapshot()
        assert np.array_equal(got_o.cpu().numpy(), oracle.adaptive_order(QT)), launch
        assert close(got_s.cpu().numpy(), sig, 1e-5)
        assert int(sc[3]) == (launch + 1) * n
    assert torch.isfinite(e.Q).all() and torch.isfinite(e.P).all() and torch.isfinite(sc).all()
    assert not e.P[0].any() and not e.Q[0].any()


def test_lds_tier_follows_the_plain_kernel_at_a_small_learning_rate():
    """Same triples, same given negatives, lr small enough that one launch's staleness is second order (the top row
    takes a third of the 150 k positives: lr x updates per row is what sets it): the two kernels leave the same
    tables to 1 % of the largest update; and the tier is NOT taken where it cannot be (no hot block, a launch that
    does not fill the chip without `always`)."""
    d, n = 128, 150_000
    P, Q, indptr, indices, users, pos, rng = skewed_problem(8000, 2000, d, n, 7)
    neg = rng.integers(1, Q.shape[0], n).astype(np.int32)
    out = []
    for lds in (0, 128):
        e = make_engine(P, Q, None, (0.01, 0.02, 0.03))
        e.set_optimizer(kind=0, lr=2e-6)
        e.set_stream_opts(True, 8)
        e.set_hot_lds(lds, always=True)
        pu, pi = e.plan_epoch(dev(users), dev(pos), n, seed=3)
        back = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(users, pos))}
        ng = np.asarray([neg[back[(int(a), int(b))]] for a, b in zip(pu.cpu().numpy(), pi.cpu().numpy())], np.int32)
        e.train_stream(pu, pi, sampler=0, neg=dev(ng))
        assert (e.stream_lds_rows() > 0) == (lds > 0)
        out.append((e.P.cpu().numpy(), e.Q.cpu().numpy()))
    moved = np.abs(out[0][1] - Q).max()
    assert moved > 2e-4
    assert np.abs(out[0][1] - out[1][1]).max() < 1e-2 * moved, np.abs(out[0][1] - out[1][1]).max() / moved
    assert np.abs(out[0][0] - out[1][0]).max() < 1e-2 * moved
    # not taken: no hot block
    e = make_engine(P, Q, None, (0.01, 0.02, 0.03))
    e.set_optimizer(kind=0, lr=1e-4)
    e.set_hot_lds(128, always=True)
    e.train_stream(dev(users), dev(pos), sampler=0, neg=dev(neg))
    assert e.stream_lds_rows() == 0
    # not taken: a launch that does not fill the chip twice, unless forced
    e.set_hot_lds(128, always=False)
    e.set_stream_opts(True, 8)
    pu, pi = e.plan_epoch(dev(users[:20_000]), dev(pos[:20_000]), 20_000, seed=3)
    e.train_stream(pu, pi, sampler=0, neg=dev(neg[:20_000]))
    assert e.stream_lds_rows() == 0


# ---- G = 32 (d <= 128): two groups share a wave, and the timed instantiation lives here ------------------------------
def seen_problem(U, I, d, n, seed, light=40, heavy=None):
    """skewed_problem with a choice of seen-list lengths: light users see 1..light - 1 items, 30 % of the users
    `heavy` = (lo, hi) items if given (past BPR_HEAVY_T: the HBM bitmaps; past LIST_CAP = 512: the CSR in HBM)."""
    rng = np.random.default_rng(seed)
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    lens = rng.integers(1, light, U)
    if heavy is not None:
        lens = np.where(rng.random(U) < 0.3, rng.integers(heavy[0], heavy[1], U), lens)
    lens[0] = 0
    rows = [np.sort(rng.choice(np.arange(1, I), size=int(k), replace=False)).astype(np.int32) for k in lens]
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    users = rng.integers(1, U, n).astype(np.int32)
    pos = (1 + (rng.zipf(1.3, n) % (I - 1))).astype(np.int32)
    return P, Q, indptr, np.concatenate(rows), users, pos, rng


def stream_seq_launches(e, Po, Qo, bo, pu, pp, given, sampler, indptr, indices, reg, lds, launches=3):
    """`launches` launches of (pu, pp) on e, the oracle's sequential SGD on (Po, Qo, bo) beside them (snapshot
    refreshed between launches for the adaptive sampler); picks exact, tables within 1e-5 after every launch.
    Returns the summed oracle scalars."""
    n = len(pu)
    upl, ppl = pu.cpu().numpy(), pp.cpu().numpy()
    sco = np.zeros(4)
    sc = torch.zeros(4, device="cuda")
    for launch in range(launches):
        if sampler == 2:
            e.adaptive_refresh()
            QT, sigma = oracle.adaptive_stats(Qo)
            snap = dict(order=oracle.adaptive_order(QT), sigma=sigma, adaptive_p=0.05)
        else:
            snap = {}
        negs = dev(given) if sampler == 0 else torch.zeros_like(pu)
        e.train_stream(pu, pp, sampler=sampler, neg=negs, adaptive_p=0.05, seed=11, offset=launch * n,
                       max_inflight=lds["inflight"], scalars=sc)
        assert e.stream_lds_rows() == lds["rows"], (launch, e.stream_lds_rows())
        neg_o = given.copy() if sampler == 0 else np.zeros(n, np.int32)
        sco += oracle.train_stream_seq(Po, Qo, bo, upl, ppl, neg_o, sampler, 0.05, reg, indptr=indptr,
                                       indices=indices, seed=11, offset=launch * n, **snap)
        if sampler != 0:
            assert np.array_equal(negs.cpu().numpy(), neg_o), (launch, (negs.cpu().numpy() != neg_o).sum())
        assert close(e.Q.cpu().numpy(), Qo, 1e-5), (launch, maxerr(e.Q.cpu().numpy(), Qo))
        assert close(e.P.cpu().numpy(), Po, 1e-5), (launch, maxerr(e.P.cpu().numpy(), Po))
        if bo is not None:
            assert close(e.item_bias.cpu().numpy(), bo, 1e-5), (launch, maxerr(e.item_bias.cpu().numpy(), bo))
    assert close(sc.cpu().numpy()[:3], sco[:3], 1e-4) and int(sc[3]) == launches * n
    return sco


# (d, run_len, sampler, item_bias, seen structure, BPR_HEAVY_T, seen-list lengths of the heavy users)
G32_SEQ = [(32, 8, 2, False, "", None, None), (64, 3, 1, True, "", None, None), (128, 1, 0, True, "", None, None),
           (128, 8, 2, True, "", None, None), (128, 8, 1, False, "", None, None), (32, 1, 1, False, "list", None, None),
           (64, 8, 2, False, "list", None, None), (128, 3, 2, True, "list", None, None),
           (128, 8, 1, False, "list", None, (520, 1000)), (64, 3, 2, True, "list", None, (520, 1000)),
           (128, 8, 2, False, "", "40", (60, 250)), (32, 8, 1, True, "", "40", (60, 250)),
           (128, 8, 2, False, "list", "600", (520, 1000)), (64, 1, 1, False, "list", "600", (520, 1000))]


@pytest.mark.parametrize("d,run_len,sampler,bias,seen,heavy_t,heavy", G32_SEQ)
def test_lds_tier_sequential_equals_b1_sgd_at_g32(d, run_len, sampler, bias, seen, heavy_t, heavy, monkeypatch):
    """The G = 32 instantiations (d = 32, 64, 128: the timed one is d = 128) with one group in flight == the oracle's
    sequential SGD, sampler included, three launches in a row: picks exact, P, Q and item_bias within 1e-5 after
    every launch, the statistics within 1e-4.  8 hot rows in LDS — 3 of them never a positive, so only the negative
    path reads and marks them — and 6 more hot rows beside them; all three zones of runs (L, L / 2, L / 4) in use,
    users cut by run boundaries; seen structures: bitmap, staged list, list overflow (users past LIST_CAP = 512 search
    the CSR in HBM), heavy users' HBM bitmaps (BPR_HEAVY_T)."""
    if seen:
        monkeypatch.setenv("BPR_SEEN", seen)
    if heavy_t is not None:
        monkeypatch.setenv("BPR_HEAVY_T", heavy_t)
    I = 80 if heavy is None else (300 if heavy[1] <= 300 else 1500)
    n = 1400
    P, Q, indptr, indices, users, pos, rng = seen_problem(120, I, d, n, d * 7 + run_len + sampler, heavy=heavy)
    counts = np.bincount(pos, minlength=I)
    popular = [int(i) for i in np.argsort(-counts, kind="stable") if counts[i] > 0]
    never = [int(i) for i in rng.permutation(np.flatnonzero(counts == 0)) if i != 0]
    if len(never) < 3:  # (a small table: free three rows of their positives)
        never = popular[-3:]
        popular = popular[:-3]
        pos = np.where(np.isin(pos, never), popular[0], pos).astype(np.int32)
    hot = popular[:5] + never[:3] + popular[5:11]  # ranks 0..7 in LDS (counts = None: rank = list order)
    b = (rng.normal(0, 0.1, I).astype(np.float32)) if bias else None
    reg = (0.01, 0.02, 0.03)
    e = make_engine(P, Q, b, reg)
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(kind=0, lr=0.05)
    e.set_stream_opts(True, run_len)
    e.set_hot_items(torch.tensor(hot, dtype=torch.int32))
    e.set_hot_lds(8, always=True)
    pu, pp = e.plan_epoch(dev(users), dev(pos), chunk=n, seed=3)
    upl = pu.cpu().numpy()
    t1, t2 = hotlds_model.zones(n, run_len, 1, 12)
    runs, _, _ = hotlds_model.runs_of(n, run_len, t1, t2)
    assert 0 < t1 < t2 < n, (t1, t2)
    assert any(upl[a - 1] == upl[a] for a, _ in runs[1:])  # users cut by run boundaries
    if heavy is not None and seen == "list":
        assert (np.diff(indptr)[np.unique(upl)] > 512).any()  # list overflow in the launch
    Po, Qo, bo = P.copy(), Q.copy(), None if b is None else b.copy()
    given = rng.integers(1, I, n).astype(np.int32)
    if sampler == 0:
        assert np.isin(never[:3], given).all()
    stream_seq_launches(e, Po, Qo, bo, pu, pp, given, sampler, indptr, indices, reg, dict(inflight=1, rows=8))


@pytest.mark.parametrize("d,sampler,run_len,seen", [(32, 2, 8, ""), (64, 1, 8, ""), (128, 0, 8, ""), (128, 1, 3, ""),
                                                    (128, 2, 8, ""), (64, 2, 1, ""), (32, 1, 8, "list"),
                                                    (64, 2, 3, "list"), (128, 2, 8, "list"), (128, 1, 8, "list")])
def test_lds_tier_two_groups_per_wave_equal_the_oracle(d, sampler, run_len, seen, monkeypatch):
    """The configuration bench.py times: G = 32 with BOTH groups of a wave at work (max_inflight = 2 -> block 64,
    gpw_active = 2, grid 1: one wave, which deals run 2k to group 0 and run 2k + 1 to group 1).  The stream
    (hotlds_model.two_half_stream) gives the even runs and the odd runs disjoint users and item rows — and the
    samplers no way out of the own half — so whatever the two groups' interleaving, the launch is the oracle's
    sequential SGD over the whole stream in stream order; the two groups share the workgroup's LDS delta block
    (both halves have rows in it, and rows in the global block beside it) and the ticket.  Three launches, picks
    exact, tables within 1e-5."""
    if seen:
        monkeypatch.setenv("BPR_SEEN", seen)
    n, K = 2000, 40
    s = hotlds_model.two_half_stream(n, run_len, 12, K, 30, seed=d + sampler + run_len)
    t1, t2 = hotlds_model.zones(n, run_len, 2, 12)
    assert 0 < t1 < t2 < n
    U, I = s["U"], s["I"]
    rng = np.random.default_rng(d)
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b = rng.normal(0, 0.1, I).astype(np.float32) if sampler != 1 else None
    pos = s["pos"]
    counts = np.bincount(pos, minlength=I)
    hot_of = []
    for h in (0, 1):
        own = np.arange(1, K + 1) + h * K
        by = own[np.argsort(-counts[own], kind="stable")]
        hot_of.append(([int(x) for x in by[:5]], [int(x) for x in own[-1:]]))
        assert counts[own[-1]] == 0  # (two_half_stream: the last rows of a half are never a positive)
    # ranks 0..7 in LDS: 3 popular rows of each half and one of each half that is only ever a negative; ranks
    # 8..11 (2 + 2) beside them
    (pa, na), (pb, nb) = hot_of
    hot = pa[:3] + na + pb[:3] + nb + pa[3:] + pb[3:]
    reg = (0.01, 0.02, 0.03)
    e = make_engine(P, Q, b, reg)
    e.bind_seen_csr(dev(s["indptr"]), dev(s["indices"]))
    e.set_optimizer(kind=0, lr=0.05)
    e.set_stream_opts(True, run_len)
    e.set_hot_items(torch.tensor(hot, dtype=torch.int32))
    e.set_hot_lds(8, always=True)
    Po, Qo, bo = P.copy(), Q.copy(), None if b is None else b.copy()
    stream_seq_launches(e, Po, Qo, bo, dev(s["users"]), dev(pos), s["neg"], sampler, s["indptr"], s["indices"], reg,
                        dict(inflight=2, rows=8))


@pytest.mark.parametrize("d,I,seen,lds,want_rows", [(32, 700, "", 64, 64), (64, 700, "", 64, 64), (128, 700, "", 64, 64),
                                                    (32, 700, "list", 64, 64), (128, 700, "list", 64, 64),
                                                    (128, 20109, "", 256, 158)])
def test_lds_tier_picks_match_the_oracle_at_full_concurrency(d, I, seen, lds, want_rows, monkeypatch):
    """The LDS-tier counterpart of test_stream_picks_match_the_oracle_at_full_concurrency: lr = 0 freezes the
    tables, so the negatives a full-width launch (default 1,024-thread workgroups, every group of every wave at work)
    draws are a pure function of (seed, offset, triple index, tables): uniform picks exact, adaptive ones up to the
    rare fp32 bin-edge flips.  P and Q come back BIT-identical: a delta row laid over a group's seen bitmap would
    flush those bits into Q.  (I = 20,109, d = 128, 256 rows asked for: the bench's shape, 158 rows fit beside the
    bitmaps.)"""
    if seen:
        monkeypatch.setenv("BPR_SEEN", seen)
    U, n = 500, 20000
    P, Q, indptr, indices, users, pos, _ = rand_problem(U, I, d, 150, seed=40 + d + I, B=n)
    P *= 6
    Q *= 6
    e = make_engine(P, Q, None, (0.01, 0.01, 0.01))
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(kind=0, lr=0.0)
    e.set_stream_opts(True, 8)
    e.set_hot_rows(256)
    e.set_hot_lds(lds, always=True)
    pu, pi = e.plan_epoch(dev(users), dev(pos), n, seed=1)
    e.adaptive_refresh()
    QT, sigma = oracle.adaptive_stats(Q)
    order = oracle.adaptive_order(QT)
    pun = pu.cpu().numpy()
    for sampler in (1, 2):
        negs = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.train_stream(pu, pi, sampler=sampler, neg=negs, adaptive_p=0.03, seed=77, offset=1000)
        assert e.stream_lds_rows() == want_rows
        got = negs.cpu().numpy()
        if sampler == 1:
            assert np.array_equal(got, oracle.sample_uniform(indptr, indices, I, pun, seed=77, offset=1000))
        else:
            want, _, _ = oracle.sample_adaptive(P, sigma, order, indptr, indices, pun, 0.03, seed=77, offset=1000)
            assert (got == want).mean() > 0.995, (got == want).mean()
        for t in range(0, n, 97):
            assert got[t] != 0 and got[t] not in indices[indptr[pun[t]]:indptr[pun[t] + 1]]
        assert np.array_equal(e.P.cpu().numpy(), P) and np.array_equal(e.Q.cpu().numpy(), Q), sampler
    # a width without a FULL instantiation does not take the tier, even forced
    P2, Q2 = rand_problem(U, I, 100, 150, seed=1, B=n)[:2]
    e = make_engine(P2, Q2, None, (0.01, 0.01, 0.01))
    e.bind_seen_csr(dev(indptr), dev(indices))
    e.set_optimizer(kind=0, lr=0.0)
    e.set_stream_opts(True, 8)
    e.set_hot_lds(lds, always=True)
    pu, pi = e.plan_epoch(dev(users), dev(pos), n, seed=1)
    e.train_stream(pu, pi, sampler=1, neg=torch.zeros(n, dtype=torch.int32, device="cuda"), seed=77)
    assert e.hot_rows() > 0 and e.stream_lds_rows() == 0
