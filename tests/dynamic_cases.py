"""The committed inputs of tests/test_gpu_dynamic.py, shared with tests/test_dynamic_model_cpu.py, which shows on the
CPU that the model alone leaves at most 1 % of every case's triples undecided (none in the sequential cases): numpy
and the CPU oracle only.  The model's answers are computed once per case and cached (never written to)."""
import numpy as np

import dynamic_model as dm

SEED = 0x9E3779B97F4A7C15  # (tests/counter64_cases.py: high word non-zero, top bit set)
MS = (2, 4, 8, 16, 32)
# every group layout of the library's widths 1 .. 1024, each at a full width and at a partial one (the last lanes'
# entries past d): G = 32 with E = 1 (20: d % 4 != 0; 32), 2 (40; 64) and 4 (128); G = 64 with E = 4 (256), 8 (300; 512)
# and 16 (1000; 1024).  The rows of a draw are scored in chunks of inflight_rows(d) = 8, 4 and 2 rows at E <= 4, 8, 16.
DS = (20, 32, 40, 64, 128, 256, 300, 512, 1000, 1024)
PICK_U, PICK_I, PICK_N, PICK_SEEN = 64, 300, 2048, 30
SEQ_DS = (32, 64, 128, 256, 300, 512, 1000, 1024)
SEQ_U, SEQ_I, SEQ_N, SEQ_LR, SEQ_REG, SEQ_M = 60, 90, 400, 0.05, (0.01, 0.02, 0.03), 4
# seeds of the sequential problems, chosen on the CPU so that every one of the 400 triples is decided
SEQ_SEED = {32: 5, 64: 5, 128: 5, 256: 5, 300: 1, 512: 1, 1000: 6, 1024: 4}
# SEQ_M = 4 is ONE chunk at E = 8: the same limit at (d, M) with M over two chunks and more (8 = 4 + 4, 10 = 4 + 4 + 2),
# seeds chosen the same way
SEQ_CHUNKED = {(300, 8): 1, (512, 10): 2}
# the stand-alone kernel's grid: DYNAMIC_MAX_GRID = 2,048 blocks of 256 threads (bpr_scored_plan.h), a group of G lanes
# per draw, so ONE pass of its grid-stride loop is 2048 * 256 / 64 = 8,192 draws at G = 64 and 16,384 at G = 32.
# GRID_N[d]: two full passes and a ragged third at d = 512; one pass and an ODD tail at d = 64, where the last wave's
# second group has no draw.
GRID_PASS = {512: 8192, 64: 16384}
GRID_N = {512: 2 * 8192 + 5, 64: 16384 + 3}
GRID_M, GRID_WINDOW, GRID_SLICE = 8, 600, 4096


def group_shape(d):
    """(G, E) of width d: bpr_group_shape.h."""
    G = 32 if d <= 128 else 64
    per = (d + G - 1) // G
    return G, ((1 if per <= 1 else 2 if per <= 2 else 4) if G == 32 else (4 if per <= 4 else 8 if per <= 8 else 16))


def inflight_rows(d):
    """Candidate rows of one chunk at width d: dynamic_inflight_rows(E) of bpr_scored_plan.h."""
    E = group_shape(d)[1]
    return 8 if E <= 4 else 4 if E <= 8 else 2


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


def seq_problem(d, M=SEQ_M):
    """test_stream_sequential_limit_equals_b1_sgd's shape at width d (M: which committed seed)."""
    key = ("seq", d, M)
    if key not in _cache:
        seed = SEQ_SEED[d] if M == SEQ_M else SEQ_CHUNKED[(d, M)]
        pr = problem(SEQ_U, SEQ_I, d, 30, seed=seed, n=SEQ_N, scale=8.0 / d ** 0.5 * 0.25)
        _cache[key] = pr
    return _cache[key]


def seq_model(d, M=SEQ_M):
    """The sequential trainer on a copy of the problem: (P, Q, negatives, decided, scalars)."""
    key = ("seq_model", d, M)
    if key not in _cache:
        pr = seq_problem(d, M)
        P, Q = pr["P"].copy(), pr["Q"].copy()
        neg, dec, sc = dm.train_sequential(P, Q, None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], M,
                                           SEQ_LR, SEQ_REG, seed=9, offset=100)
        _cache[key] = (P, Q, neg, dec, sc)
    return _cache[key]


def grid_windows(d):
    """The two stretches of a GRID_N[d] launch that are compared with the model: GRID_WINDOW draws across the first
    pass boundary of the grid-stride loop, and the last GRID_WINDOW draws (the ragged tail)."""
    n, edge = GRID_N[d], GRID_PASS[d]
    return ((edge - GRID_WINDOW // 2, min(edge + GRID_WINDOW // 2, n)), (n - GRID_WINDOW, n))


def grid_problem(d):
    """The pick tables of width d (with the bias) under GRID_N[d] users."""
    key = ("grid", d)
    if key not in _cache:
        pr = dict(pick_problem(d, True))
        pr["users"] = np.random.default_rng(78).integers(1, PICK_U, size=GRID_N[d]).astype(np.int32)
        _cache[key] = pr
    return _cache[key]


def grid_model(d, window):
    """dynamic_model.sample (M = GRID_M) of the draws window = (lo, hi) of the grid case, at offset = lo."""
    key = ("grid_model", d, window)
    if key not in _cache:
        pr = grid_problem(d)
        lo, hi = window
        out = dm.sample(pr["P"], pr["Q"], pr["b"], pr["indptr"], pr["indices"], pr["users"][lo:hi], GRID_M, SEED, lo)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
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
