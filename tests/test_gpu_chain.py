"""The serving kernels' score chain (revisit-bpr_amd/csrc/bpr_topk_shared.h: k_topk, k_retrieve, k_rank, k_neighbors,
k_rerank, k_diversify) held to its exact host model, tests/chain_model.py, on the GPU — edge values included.

Every comparison is on ids and on score BITS (chain_model.bits: int32 patterns, all NaNs as one); there is no
tolerance anywhere.  What the model is worth is measured on the CPU (tests/test_chain_model_cpu.py: its fma against
exact rational arithmetic; another chain order changes 27 - 86 % of these very scores, classes a and b).

Shapes are the smallest at which each path exists: 65 rows in a call (two user tiles: 64 + 1), 257 items (tiles of
128, 128 and 1), d = 1, 7, 33 on the element-load path and 8, 100, 128 on the vector-load path, a partial block of 8
(1, 7, 33, 100), a partial chunk of 32 (all but 128) and several chunks (33, 100, 128; 1024 once).

Value classes (chain_model.value_tables, plus the special rows `case` adds):
  a  ordinary            randn
  b  wide range          randn * 2^randint(-12, 12): heavy cancellation, the sums depend on the order
  c  subnormal           class (a) times 2^-68: products and partial sums between 2^-149 and 2^-126 and below; one
                         (user, item) pair whose only product is negative and underflows onto the zero accumulator:
                         -0 where d % 32 == 0, +0 where staged zeros follow it
  d  non-finite          +inf in two item rows (users holding 0, > 0 and < 0 there score NaN, +inf, -inf, and the two
                         tie at +inf), a NaN item row, a NaN user row among ordinary users, a user with -inf who scores
                         -inf on most items, an item row of 2^70 (its sum of squares overflows), bias entries +-inf
"""
import functools

import numpy as np
import pytest
import torch

from chain_model import bits, chain_scores, cosine_scores, select_rows, value_tables
from rank_model import rank_rows

pytestmark = pytest.mark.gpu

U, I, N_ROWS = 48, 257, 65
DS = (1, 7, 8, 33, 100, 128)
CASES = [(c, d, bias) for c in "abcd" for d in DS for bias in (False, True)] + [("a", 1024, True)]
CASE_IDS = [f"{c}-d{d}-{'bias' if bias else 'nobias'}" for c, d, bias in CASES]

# special rows (ids below the table sizes; the users among them have an empty seen row)
U_ZERO_A, U_ZERO_B, U_NAN, U_NEG, U_TINY, U_PLAIN = 6, 7, 8, 11, 5, 12
CLEAR_USERS = (U_TINY, U_ZERO_A, U_ZERO_B, U_NAN, U_NEG, U_PLAIN)
J_TINY, J_TINY2, J_INF1, J_NAN, J_BIG, J_BPOS, J_BNEG, J_INF2 = 9, 10, 20, 33, 40, 50, 51, 130


def seed_of(cls, d):
    return 1000 * "abcd".index(cls) + d


def make_csr(rng):
    """Seen CSR of the kind tests/test_gpu_recommend.py builds (int64 [U+1], int32 sorted per row, items 1 .. I-1):
    user 0 has seen nothing, user 1 everything but 3 items, the special users nothing, the rest a random fifth."""
    rows = []
    for u in range(U):
        if u == 0 or u in CLEAR_USERS:
            rows.append(np.zeros(0, np.int32))
        elif u == 1:
            keep = rng.choice(np.arange(1, I), size=3, replace=False)
            rows.append(np.setdiff1d(np.arange(1, I), keep).astype(np.int32))
        else:
            rows.append(np.flatnonzero(rng.random(I - 1) < 0.2).astype(np.int32) + 1)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(cls, d, bias):
    """The inputs of one (class, d, bias) and the model's scores for them: computed once, shared by the tests, never
    written.  Asserts that the inputs hold what their class is there for BEFORE any kernel is asked."""
    c = Case()
    P, Q, b = value_tables(cls, U, I, d, seed_of(cls, d))
    rng = np.random.default_rng(seed_of(cls, d) + 7)
    last = d - 1
    if cls == "c":
        P[U_TINY], Q[J_TINY], Q[J_TINY2] = 0, 0, 0
        P[U_TINY, last] = -2.0 ** -80
        Q[J_TINY, last] = 2.0 ** -80    # the product -2^-160 underflows onto the zero accumulator: -0
        Q[J_TINY2, last] = 2.0 ** -69   # -2^-149: the smallest subnormal
        b[J_TINY], b[J_TINY2], b[J_TINY + 2] = -0.0, 0.0, 0.0
    f_inf = min(3, last)
    if cls == "d":
        Q[1:, 0] = np.abs(Q[1:, 0])      # U_NEG holds -inf in feature 0: -inf on every item but those that make a NaN
        Q[J_INF1, f_inf] = Q[J_INF2, f_inf] = np.inf
        P[U_ZERO_A, f_inf] = P[U_ZERO_B, f_inf] = 0.0   # 0 * inf
        P[U_TINY, f_inf], P[U_PLAIN, f_inf] = 1.5, -1.5
        Q[J_NAN, d // 2] = np.nan
        P[U_NAN, last] = np.nan
        P[U_NEG, 0] = -np.inf
        Q[J_BIG] = 2.0 ** 70
        b[J_BPOS], b[J_BNEG] = np.inf, -np.inf
    c.cls, c.d, c.P, c.Q, c.b = cls, d, P, Q, (b if bias else None)
    c.indptr, c.indices = make_csr(rng)
    users = rng.integers(0, U, N_ROWS).astype(np.int32)
    users[:8] = [0, 1, U_TINY, U_ZERO_A, U_ZERO_B, U_NAN, U_NEG, U_PLAIN]  # (U_NAN sits among ordinary users)
    users[N_ROWS - 1] = users[N_ROWS // 2]  # a repeat for sure, alone in the second user tile
    c.users = users
    c.S = chain_scores(P, Q, c.b)           # [U, I]: the model
    c.ok = np.ones((U, I), bool)            # eligibility with the seen CSR
    c.ok[:, 0] = False
    for u in range(U):
        c.ok[u, c.indices[c.indptr[u]:c.indptr[u + 1]]] = False
    c.ok0 = np.ones((U, I), bool)           # ... and without
    c.ok0[:, 0] = False

    S, tiny = c.S, np.float32(2.0 ** -126)
    if cls in "abc":
        assert np.isfinite(S).all()
    if cls == "c":
        sub = (np.abs(S) < tiny) & (S != 0)
        assert sub.mean() > 0.5, "class (c): the scores are subnormal"
        s = S[U_TINY, J_TINY]
        assert s == 0 and bool(np.signbit(s)) == (d % 32 == 0), "the -0 of a full last chunk, the +0 of a padded one"
        assert (d % 32 != 0) or np.signbit(S[S == 0]).any()
        assert bias or S[U_TINY, J_TINY2] == np.float32(-2.0 ** -149)
    if cls == "d":
        assert np.isnan(S[U_ZERO_A, J_INF1]) and S[U_TINY, J_INF1] == np.inf and S[U_PLAIN, J_INF2] == -np.inf
        assert S[U_TINY, J_INF1] == S[U_TINY, J_INF2]                      # two items tie at +inf
        assert np.isnan(S[:, J_NAN]).all() and np.isnan(S[U_NAN]).all()
        neg = np.isneginf(S[U_NEG]) & c.ok[U_NEG]
        assert neg.sum() >= 128 + 64, "real items at -inf fill a row of 128 to its end"
        assert (~np.isnan(S[U_NEG]) & c.ok[U_NEG]).sum() >= 128
        if bias:
            assert (S[[0, 1, U_TINY], J_BPOS] == np.inf).all() and (S[[0, 1, U_TINY], J_BNEG] == -np.inf).all()
    return c


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def expected_rows(c, k, with_csr=True, users=None):
    users = c.users if users is None else users
    ok = (c.ok if with_csr else c.ok0)[users]
    return select_rows(c.S[users], ok, k)


def check(what, got_ids, got_scores, want_ids, want_scores):
    """ids equal and score bits equal; the figures first, then the assertion"""
    gi, gs = got_ids.cpu().numpy(), got_scores.cpu().numpy()
    bad_i, bad_s = gi != want_ids, bits(gs) != bits(want_scores)
    if bad_i.any() or bad_s.any():
        at = np.argwhere(bad_i | bad_s)[:5]
        print(what, "ids differ at", int(bad_i.sum()), "scores at", int(bad_s.sum()), "of", gi.size, "first:",
              [(tuple(p), int(gi[tuple(p)]), int(want_ids[tuple(p)]), hex(int(bits(gs)[tuple(p)]) & 0xFFFFFFFF),
                hex(int(bits(want_scores)[tuple(p)]) & 0xFFFFFFFF)) for p in at])
    assert not bad_i.any() and not bad_s.any(), what


def check_bits(what, got, want):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = bits(g) != bits(want)
    if bad.any():
        at = np.argwhere(bad)[:5]
        print(what, "differs at", int(bad.sum()), "of", g.size, "first:",
              [(tuple(p), hex(int(bits(g)[tuple(p)]) & 0xFFFFFFFF), hex(int(bits(want)[tuple(p)]) & 0xFFFFFFFF))
               for p in at])
    assert not bad.any(), what


def tensors(c):
    return gpu(c.P), gpu(c.Q), gpu(c.b), gpu(c.users), gpu(c.indptr), gpu(c.indices)


# ---- 1. every pair's score: k_rerank's fmaf chain ----------------------------------------------------------------
@pytest.mark.parametrize("cls, d, bias", CASES, ids=CASE_IDS)
def test_score_candidates_gives_the_models_bits_for_every_pair(cls, d, bias):
    """The shared list 0 .. I-1: all U x I scores of the call, both layouts.  Item 0 and (with the CSR) the seen items
    are -inf; an eligible pair has the model's bits, its NaN or infinity included."""
    from revisit_bpr.rerank import LAYOUTS, rerank, score_candidates

    c = case(cls, d, bias)
    P, Q, b, users, indptr, indices = tensors(c)
    cand = torch.arange(I, dtype=torch.int32, device="cuda")
    ninf = np.float32(-np.inf)
    for layout in LAYOUTS:
        got = score_candidates(P, Q, b, users, cand, layout=layout)
        assert got.shape == (N_ROWS, I)
        check_bits(f"no CSR, layout {layout}", got, np.where(c.ok0[c.users], c.S[c.users], ninf))
        got = score_candidates(P, Q, b, users, cand, None, indptr, indices, layout=layout)
        check_bits(f"CSR, layout {layout}", got, np.where(c.ok[c.users], c.S[c.users], ninf))
        for k in (10, 128):  # and the selection over the same list: its own compact_row, its own third key
            items, scores = rerank(P, Q, b, users, cand, k, None, indptr, indices, layout=layout)
            check(f"rerank k {k} layout {layout}", items, scores, *expected_rows(c, k))
    if cls == "d":
        g = got.cpu().numpy()
        assert np.isnan(g[5, 1:]).all() and np.isnan(g[:, J_NAN][c.ok[c.users, J_NAN]]).all()
        assert np.isposinf(g[2, J_INF1]) and np.isneginf(g[7, J_INF2]) and np.isnan(g[3, J_INF1])


# ---- 2. the fused selections: k_topk, k_retrieve (MFMA) ----------------------------------------------------------
@pytest.mark.parametrize("cls, d, bias", CASES, ids=CASE_IDS)
def test_recommend_is_select_of_the_model(cls, d, bias):
    from revisit_bpr.recommend import recommend

    c = case(cls, d, bias)
    P, Q, b, users, indptr, indices = tensors(c)
    for k in (1, 10, 128):
        want = expected_rows(c, k)
        if cls == "d":
            assert (want[0][5] == -1).all()                                  # the NaN user: nothing is returned
            assert not (want[0] == J_NAN).any()                              # the NaN item: never
            if k == 128:
                assert (want[0][6] >= 0).all() and np.isneginf(want[1][6, -1])   # real -inf items to the row's end
            if k >= 10:
                both = want[0][2, :3].tolist()
                assert both.index(J_INF1) < both.index(J_INF2)               # the tie at +inf: the smaller id first
        for s in (1, 7):
            got = recommend(P, Q, b, users, k, indptr, indices, item_slices=s)
            check(f"k {k} slices {s}", got[0], got[1], *want)
    got = recommend(P, Q, b, users, 10)  # no CSR: only item 0 is left out
    check("no CSR", got[0], got[1], *expected_rows(c, 10, with_csr=False))


@pytest.mark.parametrize("cls, d, bias", CASES, ids=CASE_IDS)
def test_retrieve_is_select_of_the_model(cls, d, bias):
    from revisit_bpr.retrieve import retrieve

    c = case(cls, d, bias)
    P, Q, b, users, indptr, indices = tensors(c)
    for k in (129, 1024):
        want = expected_rows(c, k)
        if cls == "d":  # every real item at -inf keeps its id; the padding follows it
            row = want[0][6]
            m = int((row >= 0).sum())
            assert m == (129 if k == 129 else int((c.ok[U_NEG] & ~np.isnan(c.S[U_NEG])).sum())) and m >= 129
            assert np.isneginf(want[1][6, m - 1]) and (row[:m] >= 0).all() and (row[m:] == -1).all()
        for s in (0, 2):
            got = retrieve(P, Q, b, users, k, indptr, indices, item_slices=s)
            check(f"k {k} slices {s}", got[0], got[1], *want)


# ---- 3. k_rank: the target scores, and the counts they imply ------------------------------------------------------
def targets_of(c):
    """a row of targets per list row: random ids from -1 .. I + 1 (item 0, seen ones, ids out of range), and the
    special items of the class"""
    rng = np.random.default_rng(c.d + 99)
    extra = {"c": [J_TINY, J_TINY2], "d": [J_INF1, J_INF2, J_NAN, J_BPOS, J_BNEG, J_BIG]}.get(c.cls, [])
    rows = [np.concatenate([rng.integers(-1, I + 2, 5), extra, [1 + r % (I - 1)]]).astype(np.int32)
            for r in range(N_ROWS)]
    tptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return tptr, np.concatenate(rows)


@pytest.mark.parametrize("cls, d, bias", CASES, ids=CASE_IDS)
def test_rank_items_scores_are_the_models_bits(cls, d, bias):
    """score: the model's bits (-inf for an ineligible target).  rank / not_below: tests/rank_model.py over the
    model's scores, whose comparisons are numpy's, i.e. IEEE's — "a NaN score is never before or >= anything"
    (csrc/bpr_rank.hip, include/bprcore.h): a NaN target has rank = not_below = 0 and its NaN, and a NaN item counts
    for no target."""
    from revisit_bpr.ranks import rank_items

    c = case(cls, d, bias)
    P, Q, b, users, indptr, indices = tensors(c)
    tptr, titems = targets_of(c)
    with np.errstate(invalid="ignore"):
        want = rank_rows(c.S, c.users, tptr, titems, c.indptr, c.indices)
    if cls == "d":
        nan_t = np.isnan(want[2])
        assert nan_t.sum() > 30 and (want[0][nan_t] == 0).all() and (want[1][nan_t] == 0).all()
    for s in (1, 3):
        rank, not_below, score = rank_items(P, Q, b, users, gpu(tptr), gpu(titems), indptr, indices, item_slices=s)
        check_bits(f"score, slices {s}", score, want[2])
        assert np.array_equal(rank.cpu().numpy(), want[0]), s
        assert np.array_equal(not_below.cpu().numpy(), want[1]), s


# ---- 4. k_neighbors: the dot product, the norms' chain, and the two multiplications --------------------------------
def query_rows(c):
    rng = np.random.default_rng(c.d + 5)
    rows = rng.integers(0, I, N_ROWS).astype(np.int32)
    rows[:9] = [1, 2, J_TINY, J_TINY2, J_INF1, J_NAN, J_BIG, J_INF2, 0]
    rows[N_ROWS - 1] = rows[N_ROWS // 2]
    return rows


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("cls, d, bias", [x for x in CASES if not x[2] or x[1] == 1024],
                         ids=[i for x, i in zip(CASES, CASE_IDS) if not x[2] or x[1] == 1024])
def test_similar_items_is_select_of_the_model(cls, d, bias, metric):
    """similar_items(Q, rows): never the item itself, never item 0.  Cosine as bpr_neighbors.hip's header has it: a row
    with !(ss > 0) — all zeros, an ss that underflowed, a NaN — is never returned and as a query gets a padded row; an
    ss that overflowed is +inf, rn = +0, the row stays eligible and its scores are +-0 or (inf * 0) NaN."""
    from revisit_bpr.similar import similar_items

    c = case(cls, d, bias)
    rows = query_rows(c)
    ok = np.ones((N_ROWS, I), bool)
    ok[:, 0] = False
    ok[np.arange(N_ROWS), rows] = False
    if metric == "dot":
        S = chain_scores(c.Q[rows], c.Q)
    else:
        S, ok_t, ok_x = cosine_scores(c.Q[rows], c.Q)
        ok &= ok_t[None, :] & ok_x[:, None]
        if cls == "c":
            assert not ok_t[J_TINY] and not ok_x[2]  # ss underflowed to 0
            assert ((np.abs(S[ok]) > 2.0 ** -20) & (np.abs(S[ok]) < 2)).mean() > 0.9  # ... and the rest are cosines
        if cls == "d":
            assert not ok_t[J_NAN] and not ok_x[5] and ok_t[J_BIG] and ok_t[J_INF1] and ok_x[6]
            assert np.isnan(S[0, J_INF1]) and S[0, J_BIG] == 0 and (S[6, ok[6] & ~np.isnan(S[6])] == 0).all()
    tQ, trows = gpu(c.Q), gpu(rows)
    for k in (10, 128):
        want = select_rows(S, ok, k)
        for s in (1, 3):
            got = similar_items(tQ, trows, k, metric, item_slices=s)
            check(f"{metric} k {k} slices {s}", got[0], got[1], *want)


# ---- 5. class (d): a NaN user does not disturb its tile -----------------------------------------------------------
@pytest.mark.parametrize("d, bias", [(8, True), (33, False), (128, True)])
def test_a_nan_user_gets_padding_and_leaves_its_neighbours_alone(d, bias):
    from revisit_bpr.recommend import recommend
    from revisit_bpr.retrieve import retrieve

    c = case("d", d, bias)
    P, Q, b, users, indptr, indices = tensors(c)
    at = c.users == U_NAN
    assert at[5] and not at[4] and not at[6]
    without = c.users.copy()
    without[at] = U_PLAIN
    for call, k in ((recommend, 10), (recommend, 128), (retrieve, 129)):
        got = call(P, Q, b, users, k, indptr, indices)
        ref = call(P, Q, b, gpu(without), k, indptr, indices)
        gi, gs, ri, rs = (t.cpu().numpy() for t in (*got, *ref))
        assert (gi[at] == -1).all() and np.isneginf(gs[at]).all()
        assert (ri[at] >= 0).any()
        assert gi[~at].tobytes() == ri[~at].tobytes() and gs[~at].tobytes() == rs[~at].tobytes()


# ---- 6. alignment: d % 4 == 0 at a 4-byte aligned address takes the element loads, and changes nothing -------------
def off4(t):
    """the same values, contiguous, one float past a 16-byte boundary"""
    v = torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0 and v.is_contiguous() and torch.equal(v, t)
    return v


def as_bytes(*ts):
    torch.cuda.synchronize()
    return b"".join(t.cpu().numpy().tobytes() for t in ts)


@pytest.fixture(scope="module")
def aligned():
    c = case("a", 128, True)
    return (c,) + tensors(c)


def test_alignment_recommend(aligned):
    from revisit_bpr.recommend import recommend

    c, P, Q, b, users, indptr, indices = aligned
    want = as_bytes(*recommend(P, Q, b, users, 128, indptr, indices))
    assert as_bytes(*recommend(off4(P), off4(Q), b, users, 128, indptr, indices)) == want
    assert as_bytes(*recommend(off4(P), Q, b, users, 128, indptr, indices)) == want
    assert as_bytes(*recommend(P, off4(Q), b, users, 128, indptr, indices, item_slices=3)) == want


def test_alignment_rank_items(aligned):
    from revisit_bpr.ranks import rank_items

    c, P, Q, b, users, indptr, indices = aligned
    tptr, titems = (gpu(x) for x in targets_of(c))
    want = as_bytes(*rank_items(P, Q, b, users, tptr, titems, indptr, indices))
    assert as_bytes(*rank_items(off4(P), off4(Q), b, users, tptr, titems, indptr, indices)) == want
    assert as_bytes(*rank_items(off4(P), off4(Q), b, users, tptr, titems, indptr, indices, item_slices=3)) == want


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_alignment_similar(aligned, metric):
    from revisit_bpr.similar import neighbors, similar_items

    c, P, Q, b, users, indptr, indices = aligned
    rows = gpu(query_rows(c))
    want = as_bytes(*similar_items(Q, rows, 128, metric))
    assert as_bytes(*similar_items(off4(Q), rows, 128, metric)) == want
    # the queries from a table of their own: each of the two at the odd address
    X = Q.clone()
    full = as_bytes(*neighbors(X, Q, rows, 128, metric=metric))
    assert as_bytes(*neighbors(off4(X), Q, rows, 128, metric=metric)) == full
    assert as_bytes(*neighbors(X, off4(Q), rows, 128, metric=metric)) == full


def test_alignment_rerank(aligned):
    from revisit_bpr.rerank import LAYOUTS, rerank

    c, P, Q, b, users, indptr, indices = aligned
    cand = torch.arange(I, dtype=torch.int32, device="cuda")
    for layout in LAYOUTS:
        want = as_bytes(*rerank(P, Q, b, users, cand, 128, None, indptr, indices, return_scores=True, layout=layout))
        for tP, tQ in ((off4(P), off4(Q)), (off4(P), Q), (P, off4(Q))):  # (the launcher looks only at Q)
            got = rerank(tP, tQ, b, users, cand, 128, None, indptr, indices, return_scores=True, layout=layout)
            assert as_bytes(*got) == want, layout


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_alignment_diversify(aligned, metric):
    from revisit_bpr.diversify import diversify
    from revisit_bpr.recommend import recommend

    c, P, Q, b, users, indptr, indices = aligned
    pool, rel = recommend(P, Q, b, users, 100, indptr, indices)
    want = as_bytes(*diversify(Q, pool, rel, 50, lam=0.5, metric=metric, return_mmr=True))
    assert as_bytes(*diversify(off4(Q), pool, rel, 50, lam=0.5, metric=metric, return_mmr=True)) == want
