"""Every sampling entry point against the CPU oracle at 64-bit Philox counters and a 64-bit seed.

The kernels split the counter offset + position into a low and a high 32-bit word, each in its own place
(bpr_device.h `draw` / `adaptive_randoms`, the prologues of k_stream, its LDS-tier form, k_vstream, the three fold-in
kernels, the host loop of bpr_train_strict).  A kernel that dropped the high word, or added the position to the low
word without the carry, would not fault: it would hand every rank the same negatives, or repeat a run's stream after
2^32 triples.  Here every one of them draws at

    carry        2^32 - n // 2 + 3               the low word wraps in the middle of the call
    rank1        (1 << 40) + 12345               what rank 1 of a job passes from its first triple on
    rank7_carry  (7 << 40) + 2^32 - n // 2 + 3   high word non-zero, and a carry into it

under the seed 0x9E3779B97F4A7C15 (high word non-zero, top bit set: unsigned through ctypes), and must give the
oracle's picks: uniform ones exactly, adaptive ones at the share the low-offset test of the same entry point demands
(the mismatches are fp32 bin-edge flips that do not depend on the counter:
test_adaptive_mismatches_are_cdf_bin_edges_and_ceil_flips).  tests/test_counter64_cpu.py pins the oracle's own counter
arithmetic and shows, on these inputs, that a broken counter changes more than 90 % of the picks it touches.
"""
import numpy as np
import pytest

import counter64_cases as cc
import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402

SEED = cc.SEED
DIMS = [32, 128, 256]  # G = 32 with one element per lane, G = 32 with four, G = 64


def engine_for(pr, lr=0.0, reg=(0.01, 0.01, 0.01), **opt):
    e = make_engine(pr["P"], pr["Q"], None, reg)
    e.bind_seen_csr(dev(pr["indptr"]), dev(pr["indices"]))
    e.set_optimizer(kind=opt.pop("kind", 0), lr=lr, **opt)
    return e


def share(name, got, want):
    s = float((got == want).mean())
    print(f"{name}: {s:.5f} of {len(got)} picks equal the oracle's")
    return s


# ---- 1. bpr_sample_uniform, bpr_sample_adaptive ----------------------------------------------------------------------
@pytest.mark.parametrize("off_name", cc.OFFSETS)
@pytest.mark.parametrize("d", DIMS)
def test_samplers_match_the_oracle(d, off_name):
    pr = cc.stream_problem(d)
    users, n = pr["users"], len(pr["users"])
    off = cc.offset_of(off_name, n)
    e = engine_for(pr)
    e.adaptive_refresh()
    got = e.sample_uniform(dev(users), seed=SEED, offset=off).cpu().numpy()
    assert np.array_equal(got, cc.uniform(pr, users, off, tag="raw"))
    neg, fac, rnk = (t.cpu().numpy() for t in e.sample_adaptive(dev(users), pr["p"], seed=SEED, offset=off,
                                                                return_draws=True))
    neg_o, fac_o, rnk_o = cc.adaptive(pr, users, off, tag="raw")
    same = (fac == fac_o) & (rnk == rnk_o)
    print(f"sample_adaptive d={d} {off_name}: identical (factor, rank) draws {same.mean():.5f}")
    assert same.mean() > 0.998, same.mean()
    assert np.array_equal(neg[same], neg_o[same])


# ---- 2. bpr_train_stream, lr = 0, full concurrency -------------------------------------------------------------------
def frozen_stream_picks(e, pr, pu, pi, tag, off_names, label):
    """Both samplers at every offset on the frozen tables; the tables come back bit-identical."""
    n = pu.numel()
    pun = pu.cpu().numpy()
    for off_name in off_names:
        off = cc.offset_of(off_name, n)
        for sampler in (1, 2):
            negs = torch.zeros(n, dtype=torch.int32, device="cuda")
            e.train_stream(pu, pi, sampler=sampler, neg=negs, adaptive_p=pr["p"], seed=SEED, offset=off)
            got = negs.cpu().numpy()
            if sampler == 1:
                assert np.array_equal(got, cc.uniform(pr, pun, off, tag=tag)), (off_name, label)
            else:
                s = share(f"train_stream {label} {off_name}", got, cc.adaptive(pr, pun, off, tag=tag)[0])
                assert s > 0.995, (off_name, s)
    assert np.array_equal(e.P.cpu().numpy(), pr["P"]) and np.array_equal(e.Q.cpu().numpy(), pr["Q"])


@pytest.mark.parametrize("seen", ["", "list"])
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("d", DIMS)
def test_stream_picks_match_the_oracle(d, grouped, seen, monkeypatch):
    if seen:
        monkeypatch.setenv("BPR_SEEN", seen)
    pr = cc.stream_problem(d)
    n = len(pr["users"])
    e = engine_for(pr)
    if grouped:
        e.set_stream_opts(True, 8)
        pu, pi = e.plan_epoch(dev(pr["users"]), dev(pr["pos"]), n, seed=1)
    else:
        e.set_stream_opts(False, 0)
        pu, pi = dev(pr["users"]), dev(pr["pos"])
    e.adaptive_refresh()
    frozen_stream_picks(e, pr, pu, pi, "planned" if grouped else "raw", cc.OFFSETS,
                        f"d={d} grouped={grouped} seen={seen!r}")


# ---- 3. the LDS-tier instantiation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_lds_tier_picks_match_the_oracle(d):
    """96 hot rows given by `set_hot_items` (the most popular positives), the 64 most popular of them in LDS, the
    default 1,024-thread workgroups with every group of every wave at work."""
    pr = cc.stream_problem(d, lds=True)
    n = len(pr["users"])
    e = engine_for(pr)
    e.set_stream_opts(True, 8)
    counts = np.bincount(pr["pos"], minlength=pr["I"])
    hot = np.argsort(-counts, kind="stable")[:96].astype(np.int32)
    e.set_hot_items(torch.from_numpy(hot), torch.from_numpy(counts.astype(np.int64)))
    e.set_hot_lds(64, always=True)
    pu, pi = e.plan_epoch(dev(pr["users"]), dev(pr["pos"]), n, seed=1)
    e.adaptive_refresh()
    before = e.lds_launches
    frozen_stream_picks(e, pr, pu, pi, "planned", ("carry", "rank7_carry"), f"LDS tier d={d}")
    assert e.lds_launches - before == 4 and e.stream_lds_rows() > 0  # every launch ran the LDS-tier kernel


# ---- 4. the sequential limit, learning on ----------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("sampler", [1, 2])
def test_stream_sequential_limit_matches_the_oracle(sampler, cut):
    """d = 256, one group in flight: sequential SGD, step by step the oracle's B = 1 stream at rank7_carry; cut=True
    also runs the launch's epilogue (the cut of the next snapshot's keys)."""
    pr = cc.seq_problem()
    users, pos, n = pr["users"], pr["pos"], len(pr["users"])
    off = cc.offset_of("rank7_carry", n)
    reg = (0.01, 0.02, 0.03)
    e = engine_for(pr, lr=0.05, reg=reg)
    e.adaptive_refresh()
    negs = torch.zeros(n, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    e.train_stream(dev(users), dev(pos), sampler=sampler, neg=negs, adaptive_p=pr["p"], seed=SEED, offset=off,
                   max_inflight=1, scalars=sc, cut=cut)
    sigma, order = cc.snapshot(pr)
    Po, Qo = pr["P"].copy(), pr["Q"].copy()
    neg_o = np.zeros(n, np.int32)
    sco = oracle.train_stream_seq(Po, Qo, None, users, pos, neg_o, sampler, 0.05, reg, adaptive_p=pr["p"], sigma=sigma,
                                  order=order, indptr=pr["indptr"], indices=pr["indices"], seed=SEED, offset=off)
    got = negs.cpu().numpy()
    if sampler == 1:
        assert np.array_equal(got, neg_o)
    else:  # adaptive draws depend on the live (fp32-rounded) user row; allow rare edge flips
        assert share(f"sequential limit cut={cut}", got, neg_o) > 0.97
    if np.array_equal(got, neg_o):
        assert close(e.P.cpu().numpy(), Po, 1e-5), maxerr(e.P.cpu().numpy(), Po)
        assert close(e.Q.cpu().numpy(), Qo, 1e-5), maxerr(e.Q.cpu().numpy(), Qo)
        assert close(sc.cpu().numpy()[:3], sco[:3], 1e-4)


# ---- 5. bpr_train_stream_batched -------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["sgd", "adam_01"])
@pytest.mark.parametrize("sampler", [1, 2])
def test_batched_stream_sequential_limit_matches_the_oracle(opt_name, sampler):
    """One group walks the stream: the reference's mini-batch loop on the oracle's negatives at `carry` (batches of 32:
    the wrap falls inside the 24th, and every later batch starts past it)."""
    from test_gpu_vstream import OPTS, REG, agree, oracle_opt, oracle_state

    cfg = OPTS[opt_name]
    pr = cc.synthetic_problem(64, 1500)
    users, pos, n, B = pr["users"], pr["pos"], 1500, 32
    off = cc.offset_of("carry", n)
    assert cc.wrap_of(off, n) % B and cc.wrap_of(off, n) < n - B
    e = engine_for(pr, reg=REG, **cfg)
    e.alloc_opt_state()
    e.adaptive_refresh()
    neg = torch.zeros(n, dtype=torch.int32, device="cuda")
    e.train_stream_batched(dev(users), dev(pos), B, sampler=sampler, neg=neg, adaptive_p=pr["p"], seed=SEED, offset=off,
                           max_inflight=1)
    e.flush_lazy()
    Po, Qo = pr["P"].copy(), pr["Q"].copy()
    sigma, order = cc.snapshot(pr)
    opt, st = oracle_opt(cfg), oracle_state(Po, Qo, None)
    neg_o = np.zeros(n, np.int32)
    for k, lo in enumerate(range(0, n, B)):
        sl = slice(lo, lo + B)
        if sampler == 1:
            nb = oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"], users[sl], SEED, off + lo)
        else:
            nb, _, _ = oracle.sample_adaptive(Po, sigma, order, pr["indptr"], pr["indices"], users[sl], pr["p"], SEED,
                                              offset=off + lo)
        neg_o[sl] = nb
        oracle.step(Po, Qo, None, users[sl], pos[sl], nb, opt, k + 1, st, REG)
    same = share(f"batched sequential limit {opt_name} sampler={sampler}", neg.cpu().numpy(), neg_o)
    assert same == 1.0 if sampler == 1 else same > 0.99, same  # (test_sequential_limit_with_on_device_sampling's share)
    if same == 1.0:
        assert agree(e.P.cpu().numpy(), Po, cfg), maxerr(e.P.cpu().numpy(), Po)
        assert agree(e.Q.cpu().numpy(), Qo, cfg), maxerr(e.Q.cpu().numpy(), Qo)


@pytest.mark.parametrize("sampler", [1, 2])
def test_batched_stream_full_concurrency_picks_match_the_oracle(sampler):
    """Adam at lr = 0 freezes the tables: a chip-wide launch at rank1 draws the oracle's negatives."""
    pr = cc.vstream_full_problem()
    off = cc.offset_of("rank1", len(pr["users"]))
    e = engine_for(pr, kind=2, betas=(0.9, 0.999))
    e.alloc_opt_state()
    e.adaptive_refresh()
    pu, pi = e.shuffle_epoch(dev(pr["users"]), dev(pr["pos"]), seed=5)
    neg = torch.zeros_like(pu)
    sc = torch.zeros(4, device="cuda")
    e.train_stream_batched(pu, pi, 256, sampler=sampler, neg=neg, adaptive_p=pr["p"], seed=SEED, offset=off, scalars=sc)
    users = pu.cpu().numpy()
    want = cc.uniform(pr, users, off) if sampler == 1 else cc.adaptive(pr, users, off)[0]
    assert int(sc[3]) == len(users)
    s = share(f"batched full concurrency sampler={sampler}", neg.cpu().numpy(), want)
    assert s >= (1.0 if sampler == 1 else 0.998)  # (test_full_concurrency_picks_match_the_oracle's share)
    assert np.array_equal(e.P.cpu().numpy(), pr["P"]) and np.array_equal(e.Q.cpu().numpy(), pr["Q"])


# ---- 6. bpr_train_strict (the host's offset + lo) and bpr_step -------------------------------------------------------
def test_strict_batches_draw_the_oracles_negatives():
    """2,000 triples in batches of 256 at `carry`: the wrap falls inside the 4th batch, the host adds the later
    batches' starts to a counter that has to carry.  bpr_step returns each batch's negatives; bpr_train_strict leaves
    the last batch's in its scratch and is held to the oracle's SGD steps on the oracle's negatives through the
    tables (test_train_strict_epoch_driver's tolerance)."""
    pr = cc.synthetic_problem(64, 2000)
    users, pos, n, B = pr["users"], pr["pos"], 2000, 256
    off = cc.offset_of("carry", n)
    w = cc.wrap_of(off, n)
    assert 3 * B < w < 4 * B
    reg = (0.001, 0.002, 0.003)
    want = cc.uniform(pr, users, off)
    tu, tp = dev(users), dev(pos)
    e = engine_for(pr, lr=0.0, reg=reg)
    for lo in range(0, n, B):
        _, _, _, neg = e.step(tu[lo:lo + B], tp[lo:lo + B], sampler=1, seed=SEED, offset=off + lo)
        assert np.array_equal(neg.cpu().numpy(), want[lo:lo + B]), lo
    e = engine_for(pr, lr=0.05, reg=reg)
    scratch = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.train_strict(tu, tp, B, sampler=1, neg=scratch, seed=SEED, offset=off)
    last = n - n % B
    assert np.array_equal(scratch.cpu().numpy()[:n - last], want[last:])
    Po, Qo = pr["P"].copy(), pr["Q"].copy()
    for lo in range(0, n, B):
        oracle.step_sgd_sparse(Po, Qo, None, np.ascontiguousarray(users[lo:lo + B]), np.ascontiguousarray(pos[lo:lo + B]),
                               np.ascontiguousarray(want[lo:lo + B]), 0.05, reg)
    assert np.abs(Po - pr["P"]).max() > 1e-3
    assert close(e.P.cpu().numpy(), Po, 1e-4), maxerr(e.P.cpu().numpy(), Po)
    assert close(e.Q.cpu().numpy(), Qo, 1e-4), maxerr(e.Q.cpu().numpy(), Qo)


# ---- 7. the fold-in kernels ------------------------------------------------------------------------------------------
FOLD_OFFSETS = ("carry", "rank1")


def fold_offset(name, nnz, epochs):
    """The wrap inside the second epoch's triples: the counter runs on over epochs x nnz."""
    return cc.offset_of(name, epochs * nnz, wrap=nnz + nnz // 2 - 3)


@pytest.mark.parametrize("off_name", FOLD_OFFSETS)
@pytest.mark.parametrize("d", DIMS)
def test_fold_in_uniform_negatives_are_the_oracles(d, off_name):
    from revisit_bpr.foldin import fold_in

    pr = cc.foldin_problem(d)
    epochs = cc.FOLD_EPOCHS
    off = fold_offset(off_name, pr["nnz"], epochs)
    _, neg = fold_in(dev(pr["Q"]), dev(pr["b"]), dev(pr["indptr"]), dev(pr["indices"]), epochs=epochs, lr=0.05,
                     reg_user=0.05, init=dev(pr["P"]), seed=SEED, offset=off, return_neg=True)
    torch.cuda.synchronize()
    want = cc.uniform(pr, np.tile(pr["users_of"], epochs), off)
    assert np.array_equal(neg.cpu().numpy(), want)


@pytest.mark.parametrize("off_name", FOLD_OFFSETS)
@pytest.mark.parametrize("d", DIMS)
def test_fold_in_adaptive_negatives_are_the_oracles_for_the_initial_row(d, off_name):
    """lr = 0: the row stays the initial row, so every negative is the oracle's `sample_adaptive` draw for that row
    (frozen tables: the share of test_stream_picks_match_the_oracle_at_full_concurrency); where factor and rank are
    the oracle's, so is the negative."""
    from revisit_bpr import engine as eng
    from revisit_bpr.foldin import fold_in

    pr = cc.foldin_problem(d)
    epochs = cc.FOLD_ADAPTIVE_EPOCHS
    off = fold_offset(off_name, pr["nnz"], epochs)
    Q, P0 = dev(pr["Q"]), dev(pr["P"])
    snap_engine = eng.Engine(torch.zeros(1, d, device="cuda"), Q.clone(), None, pad_user=None)
    snap_engine.adaptive_refresh()
    snapshot = snap_engine.adaptive_snapshot()
    P, neg, fac, rnk = fold_in(Q, dev(pr["b"]), dev(pr["indptr"]), dev(pr["indices"]), epochs=epochs, lr=0.0,
                               reg_user=0.0, init=P0, seed=SEED, offset=off, sampler="adaptive", adaptive_p=pr["p"],
                               snapshot=snapshot, return_neg=True, return_draws=True)
    torch.cuda.synchronize()
    assert torch.equal(P, P0)
    neg_o, fac_o, rnk_o = cc.adaptive(pr, np.tile(pr["users_of"], epochs), off)
    neg, fac, rnk = neg.cpu().numpy(), fac.cpu().numpy(), rnk.cpu().numpy()
    assert share(f"fold_in adaptive d={d} {off_name}", neg, neg_o) > 0.995
    same = (fac == fac_o) & (rnk == rnk_o)
    assert np.array_equal(neg[same], neg_o[same])


@pytest.mark.parametrize("off_name", FOLD_OFFSETS)
@pytest.mark.parametrize("d", DIMS)
def test_fold_in_items_negatives_are_the_oracles_for_each_triples_user(d, off_name):
    from revisit_bpr.foldin_items import fold_in_items

    pr = cc.foldin_items_problem(d)
    epochs = cc.FOLD_EPOCHS
    off = fold_offset(off_name, pr["nnz"], epochs)
    out = fold_in_items(dev(pr["P"]), dev(pr["Q"]), dev(pr["b"]), dev(pr["indptr"]), dev(pr["users"]), epochs=epochs,
                        lr=0.05, reg_item=0.05, init=dev(pr["Q0"]), init_bias=dev(pr["b0"]), seed=SEED, offset=off,
                        return_neg=True, seen_indptr=dev(pr["seen_indptr"]), seen_indices=dev(pr["seen_indices"]))
    torch.cuda.synchronize()
    want = cc.uniform(pr, np.tile(pr["users"], epochs), off)
    assert np.array_equal(out[-1].cpu().numpy(), want)


# ---- 8. the Python layer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["uniform", "adaptive"])
def test_stream_trainer_of_rank_1_passes_its_rank_and_running_total(sampler):
    """fast.StreamTrainer(rank=1): every launch's offset is (1 << 40) + the triples drawn so far, on over the epoch
    boundary, under the trainer's (64-bit) seed."""
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.fast import StreamTrainer
    from test_gpu_api import build

    data = synthetic.generate(300, 200, 6000, median_per_user=12, seed=2)
    model = build(data.num_users, data.num_items, 32, {"user": 0.0016, "item": 0.0001, "neg": 0.00375}, seed=13)
    tr = StreamTrainer(model, dev(data.users), dev(data.items), dev(data.indptr), dev(data.indices), lr=0.05,
                       sampler=sampler, adaptive_p=0.05, seed=SEED, rank=1)
    calls = []
    launch = tr.engine.train_stream

    def recording(users, pos, **kw):
        calls.append((kw["offset"], kw["seed"], users.numel()))
        return launch(users, pos, **kw)

    tr.engine.train_stream = recording
    stats = [tr.train_epoch() for _ in range(2)]
    assert [s["triples"] for s in stats] == [data.nnz, data.nnz]
    assert len(calls) >= 4 and sum(c[2] for c in calls) == 2 * data.nnz
    drawn = 0
    for offset, seed, count in calls:
        assert offset == (1 << 40) + drawn and seed == SEED
        drawn += count
    assert any(0 < c[0] - (1 << 40) - data.nnz < data.nnz for c in calls)  # launches inside the second epoch


def _seen_csr(users, seen, U):
    rows = {int(u): np.unique(seen[r][seen[r] > 0]) for r, u in enumerate(users)}
    lens = np.array([len(rows.get(u, ())) for u in range(U)])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rows[u] for u in range(U) if u in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return indptr, indices


def test_samplers_with_a_64_bit_generator_seed_draw_the_oracles_stream():
    """revisit_bpr.modules.UniformSampler / AdaptiveSampler pass `generator.initial_seed()` (after `generator.seed()`
    a full 64-bit value) and their running `_drawn`."""
    from revisit_bpr.modules import AdaptiveSampler, UniformSampler
    from test_gpu_api import _seen_batch, build

    U, I, d, B, S = 400, 300, 32, 4096, 30
    users, seen = _seen_batch(U, I, B, S, seed=2)
    batch = {"user": users.cuda(), "item": torch.ones(B, 1, dtype=torch.long).cuda(), "seen_items": seen.cuda()}
    un = users.numpy().astype(np.int32)
    indptr, indices = _seen_csr(un, seen.numpy(), U)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    assert gen.initial_seed() == SEED
    sampler = UniformSampler(I, gen)
    for call in range(2):
        assert sampler._drawn == call * B
        got = sampler.sample(batch).cpu().numpy().reshape(-1)
        assert np.array_equal(got, oracle.sample_uniform(indptr, indices, I, un, SEED, call * B)), call
    model = build(U, I, d, None, seed=5)
    sampler = AdaptiveSampler(model, I, sampling_prob=0.05, neg_gen=gen, every=10 ** 9)
    sampler.update_stats()
    feats = model.logits_model.get_features()
    P, Q = feats["user"].detach().cpu().numpy(), feats["item"].detach().cpu().numpy()
    QT, sigma = oracle.adaptive_stats(Q)
    order = oracle.adaptive_order(QT)
    for call in range(2):
        assert sampler._drawn == call * B
        got = sampler.sample(batch).cpu().numpy().reshape(-1)
        want, _, _ = oracle.sample_adaptive(P, sigma, order, indptr, indices, un, 0.05, SEED, call * B)
        assert share(f"AdaptiveSampler call {call}", got, want) > 0.995  # (frozen tables)


# ---- 9. seeds that differ only in the high word ----------------------------------------------------------------------
def test_plan_epoch_and_shuffle_epoch_read_the_high_word_of_the_seed():  # (exactly: tests/test_gpu_plan.py)
    from revisit_bpr.datasets import synthetic

    data = synthetic.generate(3000, 800, 70_000, median_per_user=15, seed=5)
    e = make_engine(np.zeros((data.num_users, 8), np.float32), np.zeros((data.num_items, 8), np.float32))
    users, pos = dev(data.users), dev(data.items)
    n, chunk = data.nnz, 9000
    key = np.sort(data.users.astype(np.int64) * data.num_items + data.items)
    plans = [tuple(t.cpu().numpy() for t in e.plan_epoch(users, pos, chunk, seed=s)) for s in (5, 5 + (1 << 32))]
    for uu, pp in plans:  # (test_plan_epoch_is_a_grouped_random_partition's properties)
        assert np.array_equal(np.sort(uu.astype(np.int64) * data.num_items + pp), key)
        for c0 in range(0, n, chunk):
            assert np.all(np.diff(uu[c0:c0 + chunk]) >= 0)
        assert 0.4 < (uu[:chunk] < data.num_users // 2).mean() < 0.6
    (u1, p1), (u2, p2) = plans
    assert not np.array_equal(u1, u2)
    k1 = set((u1[:chunk].astype(np.int64) * data.num_items + p1[:chunk]).tolist())
    k2 = set((u2[:chunk].astype(np.int64) * data.num_items + p2[:chunk]).tolist())
    assert 0.5 * chunk / n < len(k1 & k2) / chunk < 2.0 * chunk / n  # as unrelated as two different low words
    for m in (1000, 96_126):  # (test_shuffle_epoch_is_a_seeded_permutation's properties)
        u = torch.arange(m, dtype=torch.int32, device="cuda")
        i = (u * 7 + 3).to(torch.int32)
        a_u, a_i = e.shuffle_epoch(u, i, seed=5)
        b_u, b_i = e.shuffle_epoch(u, i, seed=5 + (1 << 32))
        for s_u, s_i in ((a_u, a_i), (b_u, b_i)):
            assert torch.equal(torch.sort(s_u).values, u) and torch.equal(s_i, (s_u * 7 + 3).to(torch.int32))
            assert float((s_u[1:] > s_u[:-1]).float().mean()) == pytest.approx(0.5, abs=0.05)
        assert not torch.equal(a_u, b_u)
        # two unrelated permutations agree in about one position (Poisson(1)): 1 % of m is ten or more of them
        assert float((a_u == b_u).float().mean()) < 0.01
