"""The committed inputs of tests/test_gpu_warp.py, shared with tests/test_warp_model_cpu.py, which shows on the CPU
that the model alone leaves at most 1 % of every case's triples undecided (none in the sequential cases): numpy and
the CPU oracle only.  The model's answers are computed once per case and cached (never written to).

Score scales.  Tables fresh from init make every candidate violate at once (all scores far inside the margin).  So the
tables here give scores of standard deviation 0.05 — those users' draws all end at tries = 1 — and every second user's
row is scaled up to a standard deviation of 4: there the positive's RANK decides, and early violators, late violators
and skipped triples all occur."""
import numpy as np

import dynamic_cases as dc
import dynamic_model as dm
import warp_model as wm

SEED = dc.SEED
MARGIN = 1.0
NS = (1, 2, 10, 32)
# every group layout of the library's widths 1 .. 1024 (tests/dynamic_cases.py: DS), each at a full width and at a
# partial one: G = 32 with E = 1 (20: no multiple of 4; 32), 2 (40; 64) and 4 (128); G = 64 with E = 4 (256), 8 (300; 512)
# and 16 (1000; 1024) — chunks of 8, 4 and 2 candidate rows
DS = (20, 32, 40, 64, 128, 256, 300, 512, 1000, 1024)
PICK_U, PICK_I, PICK_N, PICK_SEEN = 64, 300, 1024, 30
SEQ_DS = (32, 128, 256, 300, 512, 1000, 1024)
SEQ_U, SEQ_I, SEQ_N, SEQ_LR, SEQ_REG, SEQ_MAX = 60, 90, 400, 0.05, (0.01, 0.02, 0.03), 4
# seeds of the sequential problems, chosen on the CPU so that every one of the 400 triples is decided
SEQ_SEED = {32: 5, 128: 5, 256: 5, 300: 1, 512: 2, 1000: 1, 1024: 3}
# SEQ_MAX = 4 is ONE chunk at E = 8: the same limit at (d, N) with N over two chunks and more (8 = 4 + 4, 10 = 4 + 4 + 2),
# seeds chosen the same way
SEQ_CHUNKED = {(300, 8): 2, (512, 10): 3}
# the grid-stride pass and the ragged tail of the stand-alone kernel: tests/dynamic_cases.py GRID_PASS, GRID_N
GRID_MAX = 10

_cache = {}


def problem(U, I, d, per_user, seed, n, bias=False, small=0.05, large=4.0, every=2):
    """Tables with scores of standard deviation `small`, `large` for the users u % every == 0 (rows 0 zero: the pad
    rows), up to `per_user` seen items per user, n (user, positive) pairs."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    P = (rng.standard_normal((U, d)) * (small / d ** 0.5)).astype(np.float32)
    P[::every] *= np.float32(large / small)
    P[0] = 0
    Q[0] = 0
    rows = [np.sort(rng.choice(np.arange(1, I), size=int(rng.integers(per_user // 2, per_user + 1)), replace=False))
            for _ in range(U)]
    rows[0] = np.zeros(0, np.int64)
    indptr, indices = dc.csr(rows)
    users = rng.integers(1, U, size=n).astype(np.int32)
    pos = rng.integers(1, I, size=n).astype(np.int32)
    b = (rng.standard_normal(I) * 0.3).astype(np.float32) if bias else None
    return dict(P=P, Q=Q, b=b, indptr=indptr, indices=indices, users=users, pos=pos, I=I, d=d)


def pick_problem(d, bias):
    key = ("pick", d, bias)
    if key not in _cache:
        pr = problem(PICK_U, PICK_I, d, PICK_SEEN, seed=2000 + d, n=PICK_N, bias=True)
        # (the same tables with and without the bias; users, positives and seen lists — and so the accepted lists —
        # do not depend on d)
        base = problem(PICK_U, PICK_I, 4, PICK_SEEN, seed=1999, n=PICK_N)
        pr.update(users=base["users"], pos=base["pos"], indptr=base["indptr"], indices=base["indices"])
        if not bias:
            pr["b"] = None
        _cache[key] = pr
    return _cache[key]


def pick_lists():
    """The accepted lists of the pick cases for N = 32 (every smaller N is a prefix)."""
    if "lists" not in _cache:
        pr = pick_problem(32, False)
        _cache["lists"] = dm.accepted_lists(pr["indptr"], pr["indices"], PICK_I, pr["users"], 32, SEED, 0)
    return _cache["lists"]


def pick_model(N, d, bias):
    """warp_model.sample of a pick case: (items, tries, x_pos, x_neg, undecided, eps, accepted)."""
    key = ("pick_model", N, d, bias)
    if key not in _cache:
        pr = pick_problem(d, bias)
        out = wm.sample(pr["P"], pr["Q"], pr["b"], pr["indptr"], pr["indices"], pr["users"], pr["pos"], N, MARGIN, SEED,
                        0, lists=pick_lists())
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def weights_problem():
    """The d = 32 pick case with item weights bound: (problem, weights, accept, alias)."""
    import oracle

    if "weights" not in _cache:
        pr = dict(pick_problem(32, True))
        w = (np.random.default_rng(1).random(PICK_I) ** 3).astype(np.float32)
        accept, alias = oracle.alias_table(w)
        _cache["weights"] = (pr, w, accept, alias)
    return _cache["weights"]


def weights_model(N):
    key = ("weights_model", N)
    if key not in _cache:
        pr, _, accept, alias = weights_problem()
        _cache[key] = wm.sample(pr["P"], pr["Q"], pr["b"], pr["indptr"], pr["indices"], pr["users"], pr["pos"], N, MARGIN,
                                SEED, 0, accept, alias)
    return _cache[key]


def big_problem():
    """I = 70,000 at d = 20: the staged sorted list in place of the bitmap."""
    if "big" not in _cache:
        _cache["big"] = problem(16, 70_000, 20, 40, seed=31, n=256)
    return _cache["big"]


def big_model(N=10):
    key = ("big_model", N)
    if key not in _cache:
        pr = big_problem()
        _cache[key] = wm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], N, MARGIN,
                                SEED, 0)
    return _cache[key]


def seq_problem(d, N=SEQ_MAX):
    key = ("seq", d, N)
    if key not in _cache:
        seed = SEQ_SEED[d] if N == SEQ_MAX else SEQ_CHUNKED[(d, N)]
        _cache[key] = problem(SEQ_U, SEQ_I, d, 30, seed=seed, n=SEQ_N, small=0.05, large=2.0)
    return _cache[key]


def seq_model(d, N=SEQ_MAX):
    """The sequential trainer on a copy of the problem: (P, Q, negatives, tries, undecided, scalars)."""
    key = ("seq_model", d, N)
    if key not in _cache:
        pr = seq_problem(d, N)
        P, Q = pr["P"].copy(), pr["Q"].copy()
        neg, tries, und, sc = wm.train_sequential(P, Q, None, pr["indptr"], pr["indices"], pr["users"], pr["pos"],
                                                  N, MARGIN, SEQ_LR, SEQ_REG, seed=9, offset=100)
        _cache[key] = (P, Q, neg, tries, und, sc)
    return _cache[key]


def grid_problem(d):
    """The pick tables of width d (with the bias) under dynamic_cases.GRID_N[d] (user, positive) pairs."""
    key = ("grid", d)
    if key not in _cache:
        pr = dict(pick_problem(d, True))
        rng = np.random.default_rng(79)
        pr["users"] = rng.integers(1, PICK_U, size=dc.GRID_N[d]).astype(np.int32)
        pr["pos"] = rng.integers(1, PICK_I, size=dc.GRID_N[d]).astype(np.int32)
        _cache[key] = pr
    return _cache[key]


def grid_model(d, window):
    """warp_model.sample (N = GRID_MAX) of the draws window = (lo, hi) of the grid case, at offset = lo."""
    key = ("grid_model", d, window)
    if key not in _cache:
        pr = grid_problem(d)
        lo, hi = window
        out = wm.sample(pr["P"], pr["Q"], pr["b"], pr["indptr"], pr["indices"], pr["users"][lo:hi], pr["pos"][lo:hi],
                        GRID_MAX, MARGIN, SEED, lo)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def order_problem(n=2048, I=41, d=32):
    """Score of item a = a for user 1, who has seen item 1; the positive is item 38 and the margin 1.5, so items
    37 .. 40 violate: a tenth of the candidates, no score near a bound."""
    P = np.zeros((2, d), np.float32)
    P[1, 0] = 1.0
    Q = np.zeros((I, d), np.float32)
    Q[1:, 0] = np.arange(1, I)
    indptr, indices = np.array([0, 0, 1], np.int64), np.array([1], np.int32)
    return dict(P=P, Q=Q, b=None, indptr=indptr, indices=indices, I=I, d=d, users=np.full(n, 1, np.int32),
                pos=np.full(n, 38, np.int32))


def order_lists(n=2048):
    """The accepted lists (N = 32, seed 5) of the order problem: they depend on neither d nor the tables."""
    key = ("order_lists", n)
    if key not in _cache:
        pr = order_problem(n)
        _cache[key] = dm.accepted_lists(pr["indptr"], pr["indices"], pr["I"], pr["users"], 32, 5, 0)
    return _cache[key]


def skip_problem(d=32, n=256):
    """Users 1 .. 8 are SKIPPED at every N: their rows are 10 e_0, their positive is item TOP = 50 e_0 (score 500, every
    other item scores below 60), and everybody has seen TOP, so no draw touches it.  The other users are the small /
    large mix.  With an item bias."""
    key = ("skip", d, n)
    if key not in _cache:
        pr = problem(40, 120, d, 20, seed=77, n=n, bias=True)
        top, skipped = 77, np.arange(1, 9)
        pr["Q"][top] = 0
        pr["Q"][top, 0] = 50.0
        pr["b"][top] = 0.25
        pr["P"][skipped] = 0
        pr["P"][skipped, 0] = 10.0
        rows = [pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]] for u in range(40)]
        rows = [np.zeros(0, np.int64)] + [np.union1d(r, [top]) for r in rows[1:]]
        pr["indptr"], pr["indices"] = dc.csr(rows)
        order = np.argsort(pr["users"], kind="stable")
        pr["users"] = pr["users"][order]
        pr["pos"] = np.where(np.isin(pr["users"], skipped), top, pr["pos"][order]).astype(np.int32)
        pr["pos"][(pr["pos"] == top) & ~np.isin(pr["users"], skipped)] = 5
        pr.update(top=top, skipped=skipped)
        _cache[key] = pr
    return _cache[key]


def skip_model(N=10, d=32):
    """The sequential trainer on the skip problem: (P, Q, bias, negatives, tries, undecided, scalars)."""
    key = ("skip_model", N, d)
    if key not in _cache:
        pr = skip_problem(d)
        P, Q, b = pr["P"].copy(), pr["Q"].copy(), pr["b"].copy()
        neg, tries, und, sc = wm.train_sequential(P, Q, b, pr["indptr"], pr["indices"], pr["users"], pr["pos"], N, MARGIN,
                                                  SEQ_LR, SEQ_REG, seed=3, offset=2 ** 32 - 100)
        _cache[key] = (P, Q, b, neg, tries, und, sc)
    return _cache[key]


def one_unseen(I=5000, n=64, d=32):
    """User 1 has seen all but ONE of the I - 1 items (n_unseen = 1: every stepped triple has L = log 1 = 0), user 2
    has seen all of them (item 0 comes back), user 3 all but three (fewer than N unseen items).  About 0.8 of 4,096
    candidates are accepted for user 1, so both "fewer than N" and "none: the rank pick" occur over n triples.  Small
    scores: the one unseen item always violates."""
    key = ("one", I, n, d)
    if key not in _cache:
        pr = problem(4, I, d, 10, seed=3, n=n, every=99)
        unseen = 57
        rows = [np.zeros(0, np.int64), np.array([i for i in range(1, I) if i != unseen]), np.arange(1, I),
                np.array([i for i in range(1, I) if i not in (11, 22, 33)])]
        pr["indptr"], pr["indices"] = dc.csr(rows)
        pr.update(unseen=unseen, users=np.full(n, 1, np.int32))
        _cache[key] = pr
    return _cache[key]
