"""Heavy users' seen bitmaps staged in LDS (csrc/bpr_stream.h, csrc/bpr_device.h: heavy_stage), and walks of several
trips over them (the cases a walk that loads its order vectors ahead of their use has to get right).

Staging may not change a result: the same bitmap bits are read, only from a nearer place.  So, with one group in
flight (the oracle's sequential SGD, `oracle.train_stream_seq`), at a heavy threshold
of 4 so that tiny users are heavy:
  * the negatives are the oracle's, triple for triple (exact), and P, Q and item_bias are the oracle's to the 1e-5
    the sequential tests hold the kernel to (tests/test_gpu_hotlds.py::test_lds_tier_sequential_equals_b1_sgd,
    tests/test_gpu_parity.py::test_stream_runs_sequential_equals_b1_sgd: GPU and C arithmetic differ in the last
    bits of expf and of the dot product's order);
  * the same launch with the heavy table off (threshold -1), on, and on with a byte cap that pushes the lightest
    heavy users back to the build loop gives BIT-identical negatives and tables;
  * the table each launch used is the one asked for (`Engine.heavy_users`: its user count and final threshold),
    so the staged path did run where the test says it did.
Shapes: d = 32, 128 (G = 32) and 256 (G = 64); I = 200 and 2,049 (the bitmap row's last word partly used, W padded
past it: 7 -> 8 and 65 -> 68 words); the plain kernel and the LDS tier.  Seen counts: 0, the threshold, the
threshold + 1, I - 2 (one unseen item: the walk runs to the far end of its column), and users whose seen set is
exactly the first 128 / 129 / 257 entries of a factor's order from the walk's end (2 / 2 / 3 trips; at I = 200 the
second trip is the column's last: the vector after it lies wholly past the end).  Run orders: heavy -> light ->
heavy inside one run, a heavy user cut by a run boundary, both groups of a wave at work with heavy and light users
side by side (hotlds_model.two_half_stream), and a partial snapshot (the PART walk).
"""
import functools

import numpy as np
import pytest

import hotlds_model
import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402

T = 4          # heavy threshold of these tests: more than 4 seen items = heavy
L = 8          # run length
REG = (0.01, 0.02, 0.03)
LR, ADAPTIVE_P, SEED, OFFSET = 0.05, 0.05, 11, 5
HOT = list(range(1, 15))  # the hot block's rows (the LDS tier keeps 8 of them in LDS)


def seen_words(I):
    return ((I + 31) // 32 + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def problem(d, I):
    """Tables, seen CSR and a user-grouped stream with the seen counts and run orders of the module docstring; the
    oracle's snapshot of Q (one launch: the snapshot every run samples from)."""
    rng = np.random.default_rng(1000 * d + I)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    Q[0] = 0
    QT, sigma = oracle.adaptive_stats(Q)
    order = oracle.adaptive_order(QT)
    everything = np.arange(1, I, dtype=np.int32)
    rows = [np.zeros(0, np.int32),                                          # 0: the pad user
            np.zeros(0, np.int32),                                          # 1: nothing seen
            rng.choice(everything, T, replace=False),                       # 2: at the threshold (light)
            rng.choice(everything, T + 1, replace=False),                   # 3: the lightest heavy user
            np.delete(everything, rng.integers(0, I - 1))]                  # 4: one unseen item
    pinned = {}  # user -> (factor, sign): the user's row has weight on one factor only, so the walk is that column's
    heads = [(1, 128, True), (2, 129, True), (4, 128, False), (5, 129, False)]
    if I > 300:
        heads += [(3, 257, True), (6, 257, False)]
    for f, k, top in heads:
        col = order[f] if top else order[f][::-1]
        head = col[:k]
        pinned[len(rows)] = (f, 1.0 if top else -1.0)
        rows.append(head[head != 0].astype(np.int32))
    first_random = len(rows)
    for _ in range(24):
        rows.append(rng.choice(everything, int(rng.integers(0, 12)), replace=False))
    rows = [np.sort(r).astype(np.int32) for r in rows]
    U = len(rows)
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows)
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    P[0] = 0
    for u, (f, sign) in pinned.items():
        P[u] = 0
        P[u, f] = 0.5 * sign
    hu = sorted(pinned)
    # run 0: heavy -> light -> heavy; runs 1-2: head users, one of them cut by the run boundary; then the rest
    spans = [(3, 3), (1, 2), (4, 3), (hu[0], 6), (hu[1], 5), (hu[2], 3), (2, 2)] + [(u, 4) for u in hu[3:]]
    spans += [(int(u), int(rng.integers(1, 7))) for u in rng.permutation(np.arange(first_random, U))]
    users = np.concatenate([np.full(k, u, np.int32) for u, k in spans])
    n = len(users)
    assert users[L - 1] == 4 and users[2 * L - 1] == users[2 * L] == hu[1]  # the cut user is heavy
    pos = np.where(rng.random(n) < 0.5, rng.integers(1, 15, n), rng.integers(1, I, n)).astype(np.int32)
    b = rng.normal(0, 0.1, I).astype(np.float32)
    return dict(P=P, Q=Q, b=b, indptr=indptr, indices=indices, users=users, pos=pos, order=order, sigma=sigma)


@functools.lru_cache(maxsize=None)
def oracle_run(d, I, sampler):
    p = problem(d, I)
    Po, Qo, bo = p["P"].copy(), p["Q"].copy(), p["b"].copy()
    neg = np.zeros(len(p["users"]), np.int32)
    oracle.train_stream_seq(Po, Qo, bo, p["users"], p["pos"], neg, sampler, LR, REG, adaptive_p=ADAPTIVE_P,
                            sigma=p["sigma"], order=p["order"], indptr=p["indptr"], indices=p["indices"], seed=SEED,
                            offset=OFFSET)
    return neg, Po, Qo, bo


def gpu_run(p, sampler, lds, heavy, inflight=1, run_len=L, hot=HOT, partial=False):
    """One launch; heavy = (threshold, max_bytes).  Returns (neg, P, Q, item_bias) as numpy arrays."""
    e = make_engine(p["P"], p["Q"], p["b"], REG)
    e.bind_seen_csr(dev(p["indptr"]), dev(p["indices"]))
    e.set_optimizer(kind=0, lr=LR)
    e.set_stream_opts(True, run_len)
    e.set_heavy_users(*heavy)
    if lds:
        e.set_hot_items(torch.tensor(hot, dtype=torch.int32))
        e.set_hot_lds(8, always=True)
    if partial:
        e.set_tuning("partial_snapshot", 1)
        e.set_tuning("partial_target", 4)
    e.adaptive_refresh()
    if partial:
        e.adaptive_refresh_begin()
        e.adaptive_refresh_commit()
        assert e.snapshot_partial()
    neg = torch.zeros(len(p["users"]), dtype=torch.int32, device="cuda")
    e.train_stream(dev(p["users"]), dev(p["pos"]), sampler=sampler, neg=neg, adaptive_p=ADAPTIVE_P, seed=SEED,
                   offset=OFFSET, max_inflight=inflight)
    assert e.stream_lds_rows() == (8 if lds else 0)
    torch.cuda.synchronize()
    # the table the launch used: the staged path ran (or, with the table off, did not)
    n_heavy, t_end = e.heavy_users()
    cnt = np.diff(p["indptr"])
    if heavy[0] < 0:
        assert n_heavy == 0
    else:
        t_want = capped_threshold(p["indptr"], p["Q"].shape[0], heavy[1], heavy[0]) if heavy[1] else heavy[0]
        assert t_end == t_want and n_heavy == int((cnt > t_want).sum()), (n_heavy, t_end, t_want)
        assert (cnt[p["users"]] > t_want).any()  # ... and for users of this stream
    return neg.cpu().numpy(), e.P.cpu().numpy(), e.Q.cpu().numpy(), e.item_bias.cpu().numpy()


def capped_threshold(indptr, I, max_bytes, t=T):
    """The threshold bpr_set_heavy_users ends at: doubled until the rows fit max_bytes."""
    cnt = np.diff(indptr)
    while (cnt > t).sum() * seen_words(I) >= max_bytes // 4:
        t *= 2
    return t


def check(got, want, what):
    """got: a GPU run; want: the oracle's — negatives exact, tables to the sequential tests' 1e-5 (each figure is
    printed first)."""
    for name, g, w in zip(("P", "Q", "item_bias"), got[1:], want[1:]):
        print(f"{what}: {name} max rel err {maxerr(g, w):.3g}, {int((g != w).sum())} of {g.size} entries differ")
    assert np.array_equal(got[0], want[0]), (what, int((got[0] != want[0]).sum()))
    for name, g, w in zip(("P", "Q", "item_bias"), got[1:], want[1:]):
        assert close(g, w, 1e-5), (what, name, maxerr(g, w))


def identical(a, b, what):
    for name, x, y in zip(("neg", "P", "Q", "item_bias"), a, b):
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("I", [200, 2049])
@pytest.mark.parametrize("d", [32, 128, 256])
def test_staged_heavy_bitmaps_pick_like_the_oracle(d, I, lds):
    """Adaptive sampler, one group in flight: heavy table on at threshold 4 == the oracle; off (-1) and capped
    (`max_bytes`: the lightest heavy users fall back to the build loop, the heaviest stay staged) are BIT-identical
    to on."""
    p = problem(d, I)
    want = oracle_run(d, I, 2)
    cnt = np.diff(p["indptr"])[np.unique(p["users"])]
    assert {0, T, T + 1, I - 2} <= set(cnt.tolist())
    on = gpu_run(p, 2, lds, (T, 0))
    check(on, want, f"d={d} I={I} lds={lds}")
    off = gpu_run(p, 2, lds, (-1, 0))
    identical(off, on, "heavy table off")
    max_bytes = 4 * seen_words(I) * 6  # room for 5 rows
    t_cap = capped_threshold(p["indptr"], I, max_bytes)
    assert ((cnt > T) & (cnt <= t_cap)).any() and (cnt > t_cap).any(), t_cap  # some fall back, some stay
    capped = gpu_run(p, 2, lds, (T, max_bytes))
    identical(capped, on, "heavy table capped")


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("d,I", [(128, 200), (32, 2049)])
def test_staged_heavy_bitmaps_uniform_sampler(d, I, lds):
    """The uniform sampler's lookups read the same staged bitmap."""
    p = problem(d, I)
    on = gpu_run(p, 1, lds, (T, 0))
    check(on, oracle_run(d, I, 1), f"uniform d={d} I={I} lds={lds}")
    identical(gpu_run(p, 1, lds, (-1, 0)), on, "heavy table off")


def test_partial_snapshot_walk_with_staged_bitmaps():
    """The PART walk over staged bitmaps: a partial snapshot with exact ends of 4 entries — nearly
    every walk finishes inside a bin — picks what the fully sorted snapshot picks, i.e. the oracle's."""
    p = problem(128, 2049)
    on = gpu_run(p, 2, False, (T, 0), partial=True)
    check(on, oracle_run(128, 2049, 2), "partial snapshot")
    identical(gpu_run(p, 2, False, (-1, 0), partial=True), on, "heavy table off")


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("d", [32, 128])
def test_heavy_and_light_users_side_by_side_in_a_wave(d, lds):
    """Both groups of a wave at work (max_inflight = 2) on a stream whose halves share no row, so the launch is the
    oracle's sequential SGD whatever the interleaving; every user has seen the other half's K = 40 items and 0..8
    of its own: at threshold K + 4 the two groups hold heavy and light users at the same steps."""
    K, n = 40, 2000
    s = hotlds_model.two_half_stream(n, L, 12 if lds else 0, K, 30, seed=d + lds)
    runs = s["runs"]
    assert lds or all(b - a == L for a, b in runs)  # the plain kernel's runs
    cnt = np.diff(s["indptr"])
    heavy = cnt[s["users"]] > K + 4
    pairs = [(heavy[runs[r][0]], heavy[runs[r + 1][0]]) for r in range(0, len(runs) - 1, 2)]
    assert (True, False) in pairs and (False, True) in pairs  # a heavy and a light user at the same step
    rng = np.random.default_rng(d)
    p = dict(P=rng.normal(0, 0.1, (s["U"], d)).astype(np.float32), Q=rng.normal(0, 0.1, (s["I"], d)).astype(np.float32),
             b=rng.normal(0, 0.1, s["I"]).astype(np.float32), indptr=s["indptr"], indices=s["indices"],
             users=s["users"], pos=s["pos"])
    p["P"][0] = 0
    p["Q"][0] = 0
    QT, sigma = oracle.adaptive_stats(p["Q"])
    Po, Qo, bo = p["P"].copy(), p["Q"].copy(), p["b"].copy()
    neg_o = np.zeros(n, np.int32)
    oracle.train_stream_seq(Po, Qo, bo, p["users"], p["pos"], neg_o, 2, LR, REG, adaptive_p=ADAPTIVE_P, sigma=sigma,
                            order=oracle.adaptive_order(QT), indptr=p["indptr"], indices=p["indices"], seed=SEED,
                            offset=OFFSET)
    hot = list(range(1, 7)) + list(range(K + 1, K + 7))
    on = gpu_run(p, 2, lds, (K + 4, 0), inflight=2, hot=hot)
    check(on, (neg_o, Po, Qo, bo), f"two groups d={d} lds={lds}")
    off = gpu_run(p, 2, lds, (-1, 0), inflight=2, hot=hot)
    identical(off, on, "heavy table off")  # (no row is shared: every row's updates arrive in stream order)
