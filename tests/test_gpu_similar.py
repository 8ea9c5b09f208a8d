"""The fused neighbour kernel (`bpr_neighbors_rows`, revisit-bpr_amd/csrc/bpr_neighbors.hip) and what is built on it
(revisit_bpr.similar, Engine.similar_items / similar_users, Model.similar_items / similar_users) on the GPU.

References are plain numpy in this file; they restate the header comment of include/bprcore.h.  Contract under test:
row j of T is eligible for query r if first <= j < N, j != exclude[r] and, under cosine, ss(T[j]) > 0; a cosine query
with a zero norm gets a padded row; rows sorted by score descending, ties by ascending id; short rows padded with id
-1 / score -inf; the output bits a pure function of the inputs (not of n, of a query's place in the list, of the
slicing of the table); no [n, N] buffer.  Shapes are tile edges (64 queries, 128 table rows, 32 features), not
workloads."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ZERO_ROW = 7  # an all-zero table row beyond id 0 (tables of at least 8 rows)


def gpu(x):
    return None if x is None else torch.from_numpy(x).cuda()


def run(X, T, rows, k, metric, exclude=None, first=0, item_slices=0):
    from revisit_bpr.similar import neighbors

    tT = gpu(T)
    tX = tT if X is T else gpu(X)
    ids, scores = neighbors(tX, tT, gpu(rows), k, metric=metric, exclude=gpu(exclude), first=first,
                            item_slices=item_slices)
    torch.cuda.synchronize()
    assert ids.shape == scores.shape == (len(rows), k) and ids.dtype == torch.int32 and scores.dtype == torch.float32
    return ids.cpu().numpy(), scores.cpu().numpy()


def as_bytes(ids, scores):
    return ids.tobytes() + scores.tobytes()


def eligible(N, n, exclude, first):
    ok = np.ones((n, N), bool)
    ok[:, :first] = False
    if exclude is not None:
        for r, e in enumerate(exclude):
            if e >= 0:
                ok[r, e] = False
    return ok


def select(S, ok, k):
    """rows of S (float32 [n, N]) -> the k best eligible ids by (score descending, id ascending), padded"""
    n, N = S.shape
    ids = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, np.float32)
    allid = np.arange(N)
    for r in range(n):
        e = allid[ok[r]]
        top = e[np.lexsort((e, -S[r, e].astype(np.float64)))][:k]
        ids[r, :len(top)] = top
        scores[r, :len(top)] = S[r, top]
    return ids, scores


# ---- 1. + 2. integer tables: exact, with ties, both metrics ------------------------------------------------------
# (d, N, n, k, X is T, exclude, first): d = 1, 33 take the element-load path (d % 4 != 0), d = 100 ends in a partial
# chunk; N = 1, 2 pad; n = 63, 65 sit on either side of a query tile; N = 257, 5000 end in a partial table tile
EXACT = [
    (1, 1, 1, 1, True, "none", 0), (1, 1, 1, 1, True, "given", 1), (128, 2, 1, 10, True, "given", 0),
    (33, 2, 63, 10, False, "neg", 0), (1, 257, 65, 10, True, "given", 1), (33, 257, 63, 128, False, "none", 1),
    (100, 257, 65, 128, True, "neg", 0), (128, 5000, 65, 128, True, "given", 1), (100, 5000, 63, 10, False, "given", 3),
    (1024, 257, 65, 10, True, "given", 1), (1024, 5000, 1, 128, False, "none", 0), (128, 5000, 1, 1, True, "neg", 1),
    (33, 5000, 65, 1, False, "given", 1),
]


def integer_case(d, N, n, same, excl, seed):
    """Tables in [-4, 4] as fp32 with an all-zero table row (ZERO_ROW) and an all-zero query; `rows` with repeats."""
    rng = np.random.default_rng(seed)
    T = rng.integers(-4, 5, (N, d)).astype(np.float32)
    if N > ZERO_ROW:
        T[ZERO_ROW] = 0
    if same:
        X = T
    else:
        X = rng.integers(-4, 5, (40, d)).astype(np.float32)
        X[3] = 0
    rows = rng.integers(0, len(X), n).astype(np.int32)
    if n > 2:
        if not same:
            rows[1] = 3  # the all-zero query
        elif N > ZERO_ROW:
            rows[1] = ZERO_ROW
        rows[n - 1] = rows[n // 2]  # a repeat for sure
    exclude = None
    if excl != "none":
        exclude = rows.copy() if same else rng.integers(0, N, n).astype(np.int32)
        if excl == "neg":
            exclude[::3] = -1
    return X, T, rows, exclude


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("d, N, n, k, same, excl, first", EXACT)
def test_exact_with_ties(d, N, n, k, same, excl, first, metric):
    """Integer tables in [-4, 4]: every partial sum of a dot product and of a sum of squares is an exact integer
    below 16 * 1024 < 2^24 whatever the order, so dot and ss are integer arithmetic.  Cosine, as the header defines
    it and numpy's float32 computes it (IEEE division, square root and multiplication, correctly rounded): rn =
    float32(1) / sqrt(float32(ss)), s = (dot * rn_t) * rn_x.  The comparison is bitwise, ids and scores."""
    X, T, rows, exclude = integer_case(d, N, n, same, excl, d * 1000 + N + n + k)
    ids, scores = run(X, T, rows, k, metric, exclude, first)
    exp_ids, exp_scores = exact_reference(X, T, rows, exclude, first, k, metric)
    # what the case is there for
    if n > 2 and N > ZERO_ROW:
        assert not X[rows[1]].any()  # the all-zero query ...
        if metric == "cosine":
            assert (exp_ids[1] == -1).all() and (exp_ids != ZERO_ROW).all()  # ... a padded row; the zero row never
        elif k == 128 and N == 257:
            hit = exp_ids == ZERO_ROW
            assert hit.any() and (exp_scores[hit] == 0).all()  # dot: the zero row is eligible, with score 0
    if N < k:
        assert (exp_ids == -1).any()  # padding is exercised
    assert np.array_equal(ids, exp_ids)
    assert np.array_equal(scores.view(np.int32), exp_scores.view(np.int32))


def exact_reference(X, T, rows, exclude, first, k, metric):
    N, n = len(T), len(rows)
    Xq = X[rows]
    dot = np.rint(Xq.astype(np.float64) @ T.T.astype(np.float64)).astype(np.int64).astype(np.float32)
    ok = eligible(N, n, exclude, first)
    if metric == "cosine":
        ss_t = (T.astype(np.int64) ** 2).sum(1).astype(np.float32)
        ss_x = (Xq.astype(np.int64) ** 2).sum(1).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            rn_t, rn_x = np.float32(1) / np.sqrt(ss_t), np.float32(1) / np.sqrt(ss_x)
            S = (dot * rn_t[None, :]) * rn_x[:, None]
        assert S.dtype == np.float32
        ok &= (ss_t > 0)[None, :]
        ok &= (ss_x > 0)[:, None]
    else:
        S = dot
    return select(S, ok, k)


@pytest.mark.parametrize("d, N, n, k", [(100, 5000, 65, 128), (33, 257, 63, 10)])
def test_dot_equals_recommend_bitwise(d, N, n, k):
    """X = P, exclude = NULL, first = 1, dot: `bpr_topk_rows` without a bias and without a seen CSR, bit for bit —
    on float tables, where a different order of the chain would show."""
    from revisit_bpr.recommend import recommend

    rng = np.random.default_rng(d + N)
    P, Q = rng.standard_normal((50, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)
    users = rng.integers(0, 50, n).astype(np.int32)
    want = recommend(gpu(P), gpu(Q), None, gpu(users), k)
    torch.cuda.synchronize()
    got = run(P, Q, users, k, "dot", None, first=1)
    assert (got[0] >= 1).all()
    assert as_bytes(*got) == as_bytes(want[0].cpu().numpy(), want[1].cpu().numpy())


# ---- 3. float tables, derived tolerance --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("init", ["randn", "trained"])
@pytest.mark.parametrize("d, N, n, k", [(128, 5000, 200, 100), (1024, 2000, 65, 10)])
def test_float_tables_within_the_fp32_bound(init, d, N, n, k, metric):
    """S in float64, u = 2^-24.
    dot: eps = d u sum_f |x_f t_f| + u |S| — tests/test_gpu_recommend.py's bound (the standard bound of an fp32 dot
    product of length d; its second term paid for the bias add there and is kept as it stands).
    cosine: S = <x, t> / (|x| |t|), eps = u (d sum_f |x_f t_f| / (|x| |t|) + (d + 8) |S|):
      - the dot product is off by at most d u sum |x_f t_f|, which the two exact norms scale;
      - ss(v) is one chain of d non-negative terms, d roundings deep: relative error <= d u; the square root halves
        it and rounds (d / 2 + 1), the division rounds (d / 2 + 2): rn(v) is within (d / 2 + 2) u of 1 / |v|,
        relatively; two norms: (d + 4) u |S|;
      - two multiplications: 2 u |S|; (d + 6) u |S| in all to first order, and 2 u |S| of slack for the higher
        orders.
    Returned scores within eps of S; rows non-increasing, ids ascending among equal scores; no duplicates, nothing
    ineligible; every eligible id left out has S <= S_kth + eps + eps_kth."""
    rng = np.random.default_rng(d + N + n + k)
    if init == "randn":
        T = rng.standard_normal((N, d)).astype(np.float32)
    else:
        T = ((rng.random((N, d)) - 0.5) / d).astype(np.float32)
    T[0] = 0
    T[ZERO_ROW] = 0
    rows = rng.integers(1, N, n).astype(np.int32)
    rows[n - 1] = rows[n // 2]
    exclude = rows.copy()
    exclude[::5] = -1  # these queries meet themselves: cosine 1
    first = 1
    ids, scores = run(T, T, rows, k, metric, exclude, first)

    T64 = T.astype(np.float64)
    u2, absTT = 2.0 ** -24, np.abs(T64).T
    norm = np.sqrt((T64 ** 2).sum(1))
    ok_all = eligible(N, n, exclude, first)
    if metric == "cosine":
        ok_all &= (norm > 0)[None, :]
    for r, q in enumerate(rows):
        raw = T64[q] @ T64.T
        mag = np.abs(T64[q]) @ absTT
        if metric == "cosine":
            with np.errstate(divide="ignore", invalid="ignore"):
                S = raw / (norm[q] * norm)
                eps = u2 * (d * mag / (norm[q] * norm) + (d + 8) * np.abs(S))
        else:
            S = raw
            eps = d * u2 * mag + u2 * np.abs(S)
        ok = ok_all[r]
        got = ids[r]
        live = got >= 0
        m = int(live.sum())
        assert m == min(k, int(ok.sum())) == k and live[:m].all()
        g, s = got[:m], scores[r, :m]
        assert len(set(g.tolist())) == m and ok[g].all()
        assert (np.abs(s.astype(np.float64) - S[g]) <= eps[g]).all()
        assert (s[:-1] >= s[1:]).all()
        same = s[:-1] == s[1:]
        assert (g[:-1][same] < g[1:][same]).all()
        rest = ok.copy()
        rest[g] = False
        kth = g[-1]
        assert (S[rest] <= S[kth] + eps[rest] + eps[kth]).all()
        if metric == "cosine" and exclude[r] < 0:
            assert g[0] == q and abs(float(s[0]) - 1.0) <= eps[q]


# ---- 4. purity, bitwise ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def float_case():
    rng = np.random.default_rng(77)
    N, d = 5000, 128
    T = rng.standard_normal((N, d)).astype(np.float32)
    T[0] = 0
    rows = rng.integers(1, N, 130).astype(np.int32)
    rows[129] = rows[64] = rows[3]  # repeats, on both sides of a query tile's edge
    return T, rows, rows.copy()


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_item_slices_do_not_change_a_bit(float_case, metric):
    T, rows, exclude = float_case
    ref = run(T, T, rows, 100, metric, exclude, 1, item_slices=1)
    assert (ref[0] >= 1).all()
    for s in (0, 2, 7, 64):
        assert as_bytes(*run(T, T, rows, 100, metric, exclude, 1, item_slices=s)) == as_bytes(*ref), s
    # short rows across slices (only 3 eligible rows of a small table): the merge pads
    small = T[:4 + 128 * 3]
    few = np.array([1, 2, 3], np.int32)
    want = run(small, small, few, 10, metric, few, len(small) - 3, item_slices=1)
    assert (want[0][:, :3] >= 0).all() and (want[0][:, 3:] == -1).all() and np.isneginf(want[1][:, 3:]).all()
    for s in (0, 2, 4):
        assert as_bytes(*run(small, small, few, 10, metric, few, len(small) - 3, item_slices=s)) == as_bytes(*want), s


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_list_shape_does_not_change_a_bit(float_case, metric):
    """One query at a time equals the list; a permuted list permutes the rows; repeated queries agree; the same call
    twice is identical."""
    T, rows, exclude = float_case
    ids, scores = run(T, T, rows, 100, metric, exclude, 1)
    for r in list(range(0, 130, 13)) + [63, 64, 65, 129]:
        one = run(T, T, rows[r:r + 1], 100, metric, exclude[r:r + 1], 1)
        assert as_bytes(*one) == as_bytes(ids[r:r + 1], scores[r:r + 1]), r
    perm = np.random.default_rng(5).permutation(len(rows))
    pi, ps = run(T, T, rows[perm], 100, metric, exclude[perm], 1)
    assert as_bytes(pi, ps) == as_bytes(ids[perm], scores[perm])
    for r in (64, 129):
        assert as_bytes(ids[r], scores[r]) == as_bytes(ids[3], scores[3])
    assert as_bytes(*run(T, T, rows, 100, metric, exclude, 1)) == as_bytes(ids, scores)


# ---- 5. public layers --------------------------------------------------------------------------------------------
def test_similar_items_and_users_and_the_engine(float_case):
    from revisit_bpr.engine import Engine
    from revisit_bpr.similar import neighbors, similar_items, similar_users

    T, rows, _ = float_case
    rng = np.random.default_rng(9)
    tQ = gpu(T)
    tP = gpu(rng.standard_normal((300, 128)).astype(np.float32))  # (user 0's row is not zero here)
    items = gpu(rows)
    users = torch.arange(0, 300, dtype=torch.int32, device="cuda")
    for metric in ("cosine", "dot"):
        it, sc = similar_items(tQ, items, 20, metric)
        assert (it != items.unsqueeze(1)).all() and (it >= 1).all()  # never the item itself, never id 0
        want = neighbors(tQ, tQ, items, 20, metric=metric, exclude=items, first=1)
        assert torch.equal(it, want[0]) and torch.equal(sc, want[1])
        us, _ = similar_users(tP, users, 20, metric)
        assert (us != users.unsqueeze(1)).all() and (us >= 0).all()
        assert (us[1:] == 0).any()  # user 0 is a user like any other
        assert (us[0] != 0).all()
    assert torch.equal(similar_items(tQ, items, 20)[1], similar_items(tQ, items, 20, "cosine")[1])  # the default
    e = Engine(tP, tQ, gpu(rng.standard_normal(len(T)).astype(np.float32)))
    for metric in ("cosine", "dot"):
        got, want = e.similar_items(items, 20, metric=metric), similar_items(tQ, items, 20, metric)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])  # (the bias plays no part)
        got, want = e.similar_users(users, 20, metric=metric), similar_users(tP, users, 20, metric)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    e.close()
    with pytest.raises(ValueError, match="out of range"):
        similar_items(tQ, torch.tensor([len(T)], dtype=torch.int32, device="cuda"), 3)
    with pytest.raises(ValueError, match="out of range"):
        neighbors(tQ, tQ, items[:1], 3, exclude=torch.tensor([len(T)], dtype=torch.int32, device="cuda"))


def test_folded_in_style_rows_find_their_copies(float_case):
    """`neighbors(Q_new, Q, arange(m), k, first=1)`: a new row that copies T[j] gets j among its maximal-score ids,
    with a cosine within 2^-22 of 1.  ss(v) is dot(v, v) bit for bit (the same chain), so the score of a copy is
    (ss * rn) * rn with rn = 1 / sqrt(ss): the rounding of the square root and of the division, each counted twice,
    and of the two multiplications, none of d's."""
    from revisit_bpr.similar import neighbors

    T, _, _ = float_case
    js = np.array([1, 127, 128, 2500, 4999], np.int64)
    tQ = gpu(T)
    Q_new = gpu(T[js].copy())
    ids, scores = neighbors(Q_new, tQ, torch.arange(len(js), device="cuda"), 10, first=1)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    for r, j in enumerate(js):
        best = ids[r][scores[r] == scores[r].max()]
        assert j in best
        assert abs(float(scores[r, 0]) - 1.0) <= 2.0 ** -22
    assert (ids >= 1).all()


def small_model(U, I, d):
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    torch.manual_seed(3)
    return BPR(fuse_forward=True, reg_alphas={"all": 0.001},
               logits_model=MF(torch.nn.Embedding(U, d, padding_idx=0), torch.nn.Embedding(I, d, padding_idx=0),
                               item_bias=True, user_bias=False)).cuda()


def test_model_similar_syncs_first():
    from revisit_bpr import engine as eng
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.similar import similar_items, similar_users

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    model = small_model(data.num_users, data.num_items, 32)
    items = torch.arange(1, data.num_items, dtype=torch.int32, device="cuda")
    users = torch.arange(1, data.num_users, dtype=torch.int32, device="cuda")
    lm = model.logits_model
    model.bind_seen_csr(gpu(data.indptr), gpu(data.indices))

    def on_tables(metric):
        sd = model.state_dict()  # syncs: the tables as they are at this step
        return (similar_items(sd["logits_model._item_emb.weight"], items, 10, metric),
                similar_users(sd["logits_model._user_emb.weight"], users, 10, metric))

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    want = on_tables("cosine")
    assert same(model.similar_items(items, 10), want[0]) and same(model.similar_users(users, 10), want[1])
    # a few Adam steps over small batches: rows touched early are behind the step count until replayed
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    tu, ti = gpu(data.users[:960].copy()), gpu(data.items[:960].copy())
    model.train_strict(opt, tu, ti, 64, eng.NEG_UNIFORM, seed=2)
    torch.cuda.synchronize()
    stale = lm._item_emb.weight.detach().clone()
    got = model.similar_items(items, 10)  # must replay first ...
    assert not torch.equal(stale, lm._item_emb.weight.detach())  # (... and there was something to replay)
    assert not same(got, similar_items(stale, items, 10))
    for metric in ("cosine", "dot"):
        want = on_tables(metric)
        assert same(model.similar_items(items, 10, metric=metric), want[0])
        assert same(model.similar_users(users, 10, metric=metric), want[1])
    assert (got[0] != 0).all() and (got[0] != items.unsqueeze(1)).all()


def test_model_similar_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        model.similar_items(torch.ones(1, dtype=torch.int32, device="cuda"), 3)
    with pytest.raises(NotImplementedError):
        model.similar_users(torch.ones(1, dtype=torch.int32, device="cuda"), 3)


# ---- 6. no [n, N] buffer -----------------------------------------------------------------------------------------
def test_no_n_by_n_buffer():
    from revisit_bpr.similar import similar_items, slices, workspace_bytes

    n, N, k, d = 20_000, 20_109, 10, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = (torch.rand(N, d, device="cuda", generator=g) - 0.5) / d
    items = torch.randint(1, N, (n,), device="cuda", generator=g, dtype=torch.int32)
    similar_items(Q, items[:64], k)  # (the library is loaded, the kernel's code is resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, scores = similar_items(Q, items, k)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    outputs = n * k * 8
    allowed = outputs + workspace_bytes(n, N, d, k, "cosine", slices(n, N, d, k)) + (1 << 20)
    print("peak growth", growth, "allowed", allowed, "scores would be", n * N * 4)
    assert growth <= allowed < n * N * 4 // 10
    it, sc = ids.cpu().numpy(), scores.cpu().numpy()
    assert (it >= 1).all() and (it != items.cpu().numpy()[:, None]).all()
    assert (np.diff(sc, axis=1) <= 0).all() and (np.abs(sc) <= 1 + 2.0 ** -20).all()
