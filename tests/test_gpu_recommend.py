"""The fused top-K kernel (`bpr_topk_rows`, revisit-bpr_amd/csrc/bpr_topk.hip) and what is built on it
(revisit_bpr.recommend, Engine.recommend, Model.recommend, evaluation.evaluate_fused) on the GPU.

References are plain numpy in this file.  Contract under test: rows sorted by score descending, ties by ascending
item id; item 0 and the user's seen items never returned; short rows padded with item -1 / score -inf; the output
bits a pure function of the inputs (not of n, of a user's place in the list, of the item slicing); no [n, I] buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_csr(U, I, rng, density=0.2):
    """Seen CSR over U users (int64 [U+1], int32 sorted per row, items 1 .. I-1): user 0 has seen nothing, user 1
    everything but (at most) 3 items, the rest a random subset."""
    rows = []
    for u in range(U):
        if u == 0 or I < 2:
            rows.append(np.zeros(0, np.int32))
        elif u == 1:
            keep = rng.choice(np.arange(1, I), size=min(3, I - 1), replace=False)
            rows.append(np.setdiff1d(np.arange(1, I), keep).astype(np.int32))
        else:
            rows.append(np.flatnonzero(rng.random(I - 1) < density).astype(np.int32) + 1)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, indices


def user_list(U, n, rng):
    """n user ids with user 0, user 1 (where they exist) and repeats among them."""
    users = rng.integers(0, U, n).astype(np.int32)
    users[0] = 0
    if n > 2:
        users[1] = min(1, U - 1)
        users[n - 1] = users[n // 2]  # a repeat for sure
    return users


def eligible(I, u, indptr, indices):
    ok = np.ones(I, bool)
    ok[0] = False
    if indptr is not None:
        ok[indices[indptr[u]:indptr[u + 1]]] = False
    return ok


def gpu(x):
    return None if x is None else torch.from_numpy(x).cuda()


def run(P, Q, b, users, k, indptr=None, indices=None, item_slices=0):
    from revisit_bpr.recommend import recommend

    items, scores = recommend(gpu(P), gpu(Q), gpu(b), gpu(users), k, gpu(indptr), gpu(indices), item_slices=item_slices)
    torch.cuda.synchronize()
    assert items.shape == scores.shape == (len(users), k) and items.dtype == torch.int32 and scores.dtype == torch.float32
    return items.cpu().numpy(), scores.cpu().numpy()


# ---- 1. exact, with ties ---------------------------------------------------------------------------------------
# (d, I, n, k, bias, csr): d = 1, 33 take the element-load path (d % 4 != 0), d = 100, 200 end in a partial chunk
EXACT = [
    (1, 1, 1, 1, False, False), (8, 1, 65, 10, True, True), (8, 2, 63, 10, True, True), (1, 257, 65, 10, True, True),
    (33, 257, 64, 100, False, True), (100, 257, 64, 100, True, True), (128, 5000, 65, 128, False, True),
    (200, 20109, 1000, 100, True, True), (256, 5000, 64, 10, True, False), (1024, 257, 65, 128, True, True),
    (128, 20109, 1, 100, True, True), (8, 257, 1000, 1, False, False), (100, 5000, 63, 128, False, False),
    (256, 20109, 63, 1, True, True), (1024, 5000, 1, 10, False, True),
]


@pytest.mark.parametrize("d, I, n, k, bias, csr", EXACT)
def test_exact_with_ties(d, I, n, k, bias, csr):
    """Integer tables in [-4, 4] and biases in [-8, 8] as fp32: every partial sum is exact whatever the order
    (|s| <= 16 * 1024 + 8 < 2^24), so the expected result is integer arithmetic and the comparison is bitwise."""
    rng = np.random.default_rng(d * 1000 + I + n + k)
    U = 40
    P = rng.integers(-4, 5, (U, d)).astype(np.float32)
    Q = rng.integers(-4, 5, (I, d)).astype(np.float32)
    b = rng.integers(-8, 9, I).astype(np.float32) if bias else None
    indptr, indices = make_csr(U, I, rng) if csr else (None, None)
    users = user_list(U, n, rng)
    items, scores = run(P, Q, b, users, k, indptr, indices)

    S = np.rint(P.astype(np.float64) @ Q.T.astype(np.float64)).astype(np.int64)  # (exact in float64 too)
    if bias:
        S += b.astype(np.int64)
    exp_items = np.full((n, k), -1, np.int32)
    exp_scores = np.full((n, k), -np.inf, np.float32)
    ids = np.arange(I)
    for r, u in enumerate(users):
        e = ids[eligible(I, u, indptr, indices)]
        top = e[np.lexsort((e, -S[u, e]))][:k]
        exp_items[r, :len(top)] = top
        exp_scores[r, :len(top)] = S[u, top].astype(np.float32)
    if csr and n > 2 and I > 4:
        assert (exp_items[1] >= 0).sum() == min(3, k)  # the user who has seen all but 3: padding is exercised
    if I == 1:
        assert (exp_items == -1).all()
    assert np.array_equal(items, exp_items)
    assert np.array_equal(scores.view(np.int32), exp_scores.view(np.int32))


# ---- 2. float tables, derived tolerance ------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["randn", "trained"])
@pytest.mark.parametrize("d, I, n, k", [(128, 5000, 200, 100), (100, 20109, 70, 128), (1024, 2000, 65, 10)])
def test_float_tables_within_the_fp32_bound(init, d, I, n, k):
    """S = P64[u] Q64^T + b in float64; eps(u, i) = d 2^-24 sum_f |p_uf q_if| + 2^-24 |S| (the standard bound of an
    fp32 dot product of length d, plus the rounding of the bias add).  Returned scores within eps of S; rows
    non-increasing, ids ascending among equal scores; no duplicates, nothing excluded; every eligible item left out
    has S(u, i) <= S(u, kth) + eps(u, i) + eps(u, kth)."""
    rng = np.random.default_rng(d + I + n + k)
    U = 60
    if init == "randn":
        P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
        b = rng.standard_normal(I).astype(np.float32)
    else:
        P, Q = ((rng.random((U, d)) - 0.5) / d).astype(np.float32), ((rng.random((I, d)) - 0.5) / d).astype(np.float32)
        b = ((rng.random(I) - 0.5) / d).astype(np.float32)
    indptr, indices = make_csr(U, I, rng)
    users = user_list(U, n, rng)
    items, scores = run(P, Q, b, users, k, indptr, indices)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    u2, absQT = 2.0 ** -24, np.abs(Q64).T
    for r, u in enumerate(users):
        S = P64[u] @ Q64.T + b
        eps = d * u2 * (np.abs(P64[u]) @ absQT) + u2 * np.abs(S)
        ok = eligible(I, u, indptr, indices)
        got = items[r]
        live = got >= 0
        m = int(live.sum())
        assert m == min(k, int(ok.sum())) and live[:m].all()  # padding only at the end, only when items run out
        assert np.isneginf(scores[r, m:]).all()
        g, s = got[:m], scores[r, :m]
        assert len(set(g.tolist())) == m and ok[g].all()
        assert (np.abs(s.astype(np.float64) - S[g]) <= eps[g]).all()
        assert (s[:-1] >= s[1:]).all()
        same = s[:-1] == s[1:]
        assert (g[:-1][same] < g[1:][same]).all()
        if m == k:
            rest = ok.copy()
            rest[g] = False
            kth = g[-1]
            assert (S[rest] <= S[kth] + eps[rest] + eps[kth]).all()


# ---- 3. invariance, bitwise ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def float_case():
    rng = np.random.default_rng(77)
    U, I, d = 300, 20109, 128
    P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
    b = rng.standard_normal(I).astype(np.float32)
    indptr, indices = make_csr(U, I, rng, density=0.02)
    users = user_list(U, 130, rng)
    return P, Q, b, users, indptr, indices


def as_bytes(items, scores):
    return items.tobytes() + scores.tobytes()


def test_item_slices_do_not_change_a_bit(float_case):
    P, Q, b, users, indptr, indices = float_case
    ref = run(P, Q, b, users, 100, indptr, indices, item_slices=1)
    assert (ref[0] >= 0).any()
    for s in (0, 2, 7, 64):
        assert as_bytes(*run(P, Q, b, users, 100, indptr, indices, item_slices=s)) == as_bytes(*ref), s
    # a short row (users[1]: the user who has seen all but 3) across slices: the merge pads
    for s in (0, 1, 2, 7):
        it, sc = run(P, Q, b, users[:3], 10, indptr, indices, item_slices=s)
        assert as_bytes(it, sc) == as_bytes(ref[0][:3, :10], ref[1][:3, :10]), s
        assert (it[1, :3] >= 0).all() and (it[1, 3:] == -1).all() and np.isneginf(sc[1, 3:]).all()


def test_one_at_a_time_equals_the_list(float_case):
    P, Q, b, users, indptr, indices = float_case
    items, scores = run(P, Q, b, users, 100, indptr, indices)
    for r in list(range(0, 130, 9)) + [63, 64, 65, 129]:
        one = run(P, Q, b, users[r:r + 1], 100, indptr, indices)
        assert as_bytes(*one) == as_bytes(items[r:r + 1], scores[r:r + 1]), r


def test_permuted_list_permutes_the_rows(float_case):
    P, Q, b, users, indptr, indices = float_case
    items, scores = run(P, Q, b, users, 100, indptr, indices)
    perm = np.random.default_rng(5).permutation(len(users))
    pi, ps = run(P, Q, b, users[perm], 100, indptr, indices)
    assert as_bytes(pi, ps) == as_bytes(items[perm], scores[perm])
    again = run(P, Q, b, users, 100, indptr, indices)
    assert as_bytes(*again) == as_bytes(items, scores)  # and the same call twice


# ---- 4. public layers ------------------------------------------------------------------------------------------
def test_engine_recommend_is_recommend_on_its_tables(float_case):
    from revisit_bpr.engine import Engine
    from revisit_bpr.recommend import recommend

    P, Q, b, users, indptr, indices = float_case
    tP, tQ, tb, tu, tptr, tidx = (gpu(x) for x in (P, Q, b, users, indptr, indices))
    e = Engine(tP, tQ, tb)
    none = e.recommend(tu, 20)  # no CSR bound: only item 0 is left out
    assert all(torch.equal(x, y) for x, y in zip(none, recommend(tP, tQ, tb, tu, 20)))
    e.bind_seen_csr(tptr, tidx)
    want = recommend(tP, tQ, tb, tu, 20, tptr, tidx)
    got = e.recommend(tu, 20)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # exclude_seen=False: seen items come back (user 1 has seen all but 3 of 20,108), item 0 never
    raw = e.recommend(tu, 20, exclude_seen=False)
    assert torch.equal(raw[0], none[0]) and torch.equal(raw[1], none[1])
    it = raw[0].cpu().numpy()
    seen1 = set(indices[indptr[1]:indptr[2]].tolist())
    assert len(seen1 & set(it[1].tolist())) >= 17 and (it != 0).all() and (it > 0).all()
    assert (got[0].cpu().numpy() != 0).all()
    e.close()


def small_model(U, I, d, user_bias):
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    torch.manual_seed(3)
    return BPR(fuse_forward=True, reg_alphas={"all": 0.001},
               logits_model=MF(torch.nn.Embedding(U, d, padding_idx=0), torch.nn.Embedding(I, d, padding_idx=0),
                               item_bias=True, user_bias=user_bias)).cuda()


@pytest.mark.parametrize("user_bias", [False, True])
def test_model_recommend_syncs_and_adds_the_user_bias(user_bias):
    from revisit_bpr import engine as eng
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.recommend import recommend

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    model = small_model(data.num_users, data.num_items, 32, user_bias)
    if user_bias:
        with torch.no_grad():
            model.logits_model._user_bias.copy_(torch.randn(data.num_users, device="cuda"))
    tptr, tidx = gpu(data.indptr), gpu(data.indices)
    model.bind_seen_csr(tptr, tidx)
    users = torch.arange(0, data.num_users, dtype=torch.int32, device="cuda")
    lm = model.logits_model

    def on_tables(exclude=True):
        sd = model.state_dict()
        it, sc = recommend(sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"],
                           sd["logits_model._item_bias"], users, 10, tptr if exclude else None,
                           tidx if exclude else None)
        if user_bias:
            sc = sc + sd["logits_model._user_bias"][users.long()].unsqueeze(1)
        return it, sc

    got = model.recommend(users, 10)
    want = on_tables()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a few Adam steps over small batches: rows touched early are behind the step count until replayed
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    tu, ti = gpu(data.users[:960].copy()), gpu(data.items[:960].copy())
    model.train_strict(opt, tu, ti, 64, eng.NEG_UNIFORM, seed=2)
    torch.cuda.synchronize()
    stale = lm._item_emb.weight.detach().clone()
    got = model.recommend(users, 10)  # must replay first ...
    assert not torch.equal(stale, lm._item_emb.weight.detach())  # (... and there was something to replay)
    want = on_tables()  # state_dict() syncs: the tables as they are at this step
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    raw, want_raw = model.recommend(users, 10, exclude_seen=False), on_tables(exclude=False)
    assert torch.equal(raw[0], want_raw[0]) and torch.equal(raw[1], want_raw[1])
    assert (raw[0] > 0).all() and not torch.equal(raw[0], got[0])


def test_model_recommend_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        model.recommend(torch.zeros(1, dtype=torch.int32, device="cuda"), 3)


# ---- 5. evaluate_fused vs evaluate_topk --------------------------------------------------------------------------
def test_evaluate_fused_equals_evaluate_topk():
    """The data of test_gpu_api.py::test_evaluate_topk_equals_metric_classes, and its tolerance."""
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.evaluation import evaluate_fused, evaluate_topk

    data = synthetic.generate_latent(700, 260, 15000, seed=8)
    g = torch.Generator().manual_seed(0)
    P = torch.randn(data.num_users, 32, generator=g).cuda()
    Q = torch.randn(data.num_items, 32, generator=g).cuda()
    b = torch.randn(data.num_items, generator=g).cuda()
    t = {k: torch.from_numpy(getattr(data, k)).cuda()
         for k in ("eval_users", "eval_indptr", "eval_items", "indptr", "indices")}
    ks = (5, 10, 20, 50, 100)
    args = (P, Q, b, t["eval_users"], t["eval_indptr"], t["eval_items"], t["indptr"], t["indices"])
    slow = evaluate_topk(*args, ks=ks, block=300)
    fast = evaluate_fused(*args, ks=ks)
    assert set(fast) == set(slow) and len(fast) == 15
    for name, v in slow.items():
        print(name, fast[name], v, fast[name] - v)
    for name, v in slow.items():
        assert abs(fast[name] - v) < 2e-6, (name, fast[name], v)
    assert 0.0 < fast["ndcg@100"] < 1.0


# ---- 6. no [n, I] buffer -----------------------------------------------------------------------------------------
def test_no_n_by_i_buffer():
    from revisit_bpr.recommend import recommend, slices, workspace_bytes

    n, I, k, d, U = 20_000, 20_109, 100, 128, 25_000
    g = torch.Generator(device="cuda").manual_seed(1)
    P = (torch.rand(U, d, device="cuda", generator=g) - 0.5) / d
    Q = (torch.rand(I, d, device="cuda", generator=g) - 0.5) / d
    b = (torch.rand(I, device="cuda", generator=g) - 0.5) / d
    users = torch.randint(0, U, (n,), device="cuda", generator=g, dtype=torch.int32)
    cnt = torch.randint(0, 40, (U,), device="cuda", generator=g)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(cnt, 0)])
    nnz = int(indptr[-1])
    # sorted, distinct items per row: a row's r-th item is 1 + 500 r + (a per-row offset below 500)
    offs = torch.arange(nnz, device="cuda") - torch.repeat_interleave(indptr[:-1], cnt)
    base = torch.repeat_interleave(torch.randint(0, 500, (U,), device="cuda", generator=g), cnt)
    indices = (1 + 500 * offs + base).to(torch.int32)
    recommend(P, Q, b, users[:64], k, indptr, indices)  # (the library is loaded, the kernel's code is resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    items, scores = recommend(P, Q, b, users, k, indptr, indices)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    outputs = n * k * 8
    allowed = outputs + workspace_bytes(n, I, d, k, slices(n, I, d, k)) + (1 << 20)  # (this call's own need: 0)
    print("peak growth", growth, "allowed", allowed, "logits would be", n * I * 4)
    assert growth <= allowed < n * I * 4 // 10
    it = items.cpu().numpy()
    assert (it > 0).all() and (np.diff(scores.cpu().numpy(), axis=1) <= 0).all()
    # spot check of the exclusion at this size
    ptr, idx, us = indptr.cpu().numpy(), indices.cpu().numpy(), users.cpu().numpy()
    for r in range(0, n, 997):
        assert not set(it[r].tolist()) & set(idx[ptr[us[r]]:ptr[us[r] + 1]].tolist())
