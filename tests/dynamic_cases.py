"""The committed inputs of tests/test_gpu_dynamic.py, shared with tests/test_dynamic_model_cpu.py, which shows on the
CPU that the model alone leaves at most 1 % of every case's triples undecided (none in the sequential cases): numpy
and the CPU oracle only.  The model's answers are computed once per case and cached (never written to)."""
import numpy as np

import dynamic_model as dm

SEED = 0x9E3779B97F4A7C15  # (tests/counter64_cases.py: high word non-zero, top bit set)
MS = (2, 4, 8, 16, 32)
DS = (20, 32, 64, 128, 256)  # every group layout up to d = 256 (E = 1, 1, 2, 4 at G = 32; 4 at G = 64), one d % 4 != 0
PICK_U, PICK_I, PICK_N, PICK_SEEN = 64, 300, 2048, 30
SEQ_DS = (32, 64, 128, 256)
SEQ_U, SEQ_I, SEQ_N, SEQ_LR, SEQ_REG, SEQ_M = 60, 90, 400, 0.05, (0.01, 0.02, 0.03), 4
# seeds of the sequential problems, chosen on the CPU so that every one of the 400 triples is decided
SEQ_SEED = {32: 5, 64: 5, 128: 5, 256: 5}


def csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, indices


def problem(U, I, d, per_user, seed, n, scale=0.5, bias=False):
    """Random tables (rows 0 zero: the pad rows), up to `per_user` seen items per user, n (user, positive) pairs."""
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((U, d)) * scale).astype(np.float32)
    Q = (rng.standard_normal((I, d)) * scale).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    rows = [np.sort(rng.choice(np.arange(1, I), size=int(rng.integers(per_user // 2, per_user + 1)), replace=False))
            for _ in range(U)]
    rows[0] = np.zeros(0, np.int64)
    indptr, indices = csr(rows)
    users = rng.integers(1, U, size=n).astype(np.int32)
    pos = rng.integers(1, I, size=n).astype(np.int32)
    b = (rng.standard_normal(I) * scale).astype(np.float32) if bias else None
    return dict(P=P, Q=Q, b=b, indptr=indptr, indices=indices, users=users, pos=pos, I=I, d=d)


_cache = {}


def pick_problem(d, bias):
    key = ("pick", d, bias)
    if key not in _cache:
        pr = problem(PICK_U, PICK_I, d, PICK_SEEN, seed=1000 + d, n=PICK_N, bias=True)
        # (the same tables with and without the bias; the users — and so the accepted lists — do not depend on d)
        users = np.random.default_rng(77).integers(1, PICK_U, size=PICK_N).astype(np.int32)
        rows = problem(PICK_U, PICK_I, 4, PICK_SEEN, seed=999, n=1)
        pr.update(users=users, indptr=rows["indptr"], indices=rows["indices"])
        if not bias:
            pr["b"] = None
        _cache[key] = pr
    return _cache[key]


def pick_lists():
    """The accepted lists of the pick cases for M = 32 (every smaller M is a prefix)."""
    if "lists" not in _cache:
        pr = pick_problem(32, False)
        _cache["lists"] = dm.accepted_lists(pr["indptr"], pr["indices"], PICK_I, pr["users"], 32, SEED, 0)
    return _cache["lists"]


def pick_model(M, d, bias):
    """dynamic_model.sample of a pick case: (items, scores, decided, margins, accepted)."""
    key = ("pick_model", M, d, bias)
    if key not in _cache:
        pr = pick_problem(d, bias)
        out = dm.sample(pr["P"], pr["Q"], pr["b"], pr["indptr"], pr["indices"], pr["users"], M, SEED, 0,
                        lists=pick_lists())
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def seq_problem(d):
    """test_stream_sequential_limit_equals_b1_sgd's shape at width d."""
    key = ("seq", d)
    if key not in _cache:
        pr = problem(SEQ_U, SEQ_I, d, 30, seed=SEQ_SEED[d], n=SEQ_N, scale=8.0 / d ** 0.5 * 0.25)
        _cache[key] = pr
    return _cache[key]


def seq_model(d):
    """The sequential trainer on a copy of the problem: (P, Q, negatives, decided, scalars)."""
    key = ("seq_model", d)
    if key not in _cache:
        pr = seq_problem(d)
        P, Q = pr["P"].copy(), pr["Q"].copy()
        neg, dec, sc = dm.train_sequential(P, Q, None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], SEQ_M,
                                           SEQ_LR, SEQ_REG, seed=9, offset=100)
        _cache[key] = (P, Q, neg, dec, sc)
    return _cache[key]


def nearly_all_seen(I=5000, n=64, d=32):
    """One user who has seen all but ONE of the I - 1 items, one who has seen all of them: about 0.8 of 4,096
    candidates are accepted for the first, so both "fewer than M" and "none: the rank pick" occur over n triples."""
    key = ("edge", I, n, d)
    if key not in _cache:
        rng = np.random.default_rng(3)
        P = (rng.standard_normal((3, d)) * 0.5).astype(np.float32)
        Q = (rng.standard_normal((I, d)) * 0.5).astype(np.float32)
        P[0] = 0
        Q[0] = 0
        unseen = 1234
        rows = [np.zeros(0, np.int64), np.array([i for i in range(1, I) if i != unseen]), np.arange(1, I)]
        indptr, indices = csr(rows)
        _cache[key] = dict(P=P, Q=Q, b=None, indptr=indptr, indices=indices, I=I, d=d, unseen=unseen,
                           users=np.full(n, 1, np.int32))
    return _cache[key]
