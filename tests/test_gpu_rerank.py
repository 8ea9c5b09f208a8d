"""The fused re-ranking kernel (`bpr_rerank_rows`, revisit-bpr_amd/csrc/bpr_rerank.hip) and what is built on it
(revisit_bpr.rerank.rerank / score_candidates, Engine.rerank, Model.rerank) on the GPU.

The yardstick is tests/rerank_model.py (brute force in numpy, pinned on the CPU by tests/test_rerank_cpu.py).
Contract under test: a candidate is eligible iff 0 < id < I and the user has not seen it; cand_scores holds the score
of every candidate (-inf: not eligible); the top k of a row's own candidates come back sorted by score descending, id
ascending, a listed-m-times id up to m times, padded with -1 / -inf; a score is `recommend`'s and `rank_items`' bits;
the outputs are a pure function of the inputs (not of the row order, the order inside a row, the split of the call or
the layout).

Shapes: T = RERANK_TILE = 256 is the workgroup layout's tile, 64 the wave layout's; rows of 63 .. 65, 255 .. 257 and
2T + 3 candidates sit on both sides of either; n = 70 rows leaves a partial last group of 4 in the wave layout;
d = 33 takes the element-load path and a padded chunk, d = 256 eight chunks."""

import numpy as np
import pytest
import torch

from rerank_model import rerank_rows

pytestmark = pytest.mark.gpu

U, I, N = 12, 300, 70
EDGE = np.array([127, 128, 129, 255, 256, 299], np.int32)
KS = (1, 10, 128)


def mod():
    from revisit_bpr import rerank

    return rerank


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(P, Q, b, users, cptr, citems, k, indptr=None, indices=None, layout=0):
    """(items, scores, cand_scores) as numpy"""
    out = mod().rerank(gpu(P), gpu(Q), gpu(b), gpu(users), gpu(citems), k, gpu(cptr), gpu(indptr), gpu(indices),
                       return_scores=True, layout=layout)
    torch.cuda.synchronize()
    assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.float32]
    assert out[0].shape == out[1].shape == (len(users), k)
    assert out[2].shape == ((len(citems),) if cptr is not None else (len(users), len(citems)))
    return tuple(o.cpu().numpy() for o in out)


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def seen_csr(rng):
    """tests/test_gpu_rank.py::seen_csr: user 0 has seen nothing, user 1 everything, user 2 exactly the items at the
    tile boundaries, user 3 those and more; the rest a random third."""
    rows = []
    for u in range(U):
        if u == 0:
            rows.append(np.zeros(0, np.int32))
        elif u == 1:
            rows.append(np.arange(1, I, dtype=np.int32))
        elif u == 2:
            rows.append(EDGE)
        else:
            r = np.flatnonzero(rng.random(I - 1) < 0.33).astype(np.int32) + 1
            rows.append(np.union1d(r, EDGE).astype(np.int32) if u == 3 else r)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def csr_of(lists):
    cptr = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    return cptr, (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int32)


ALL_SEEN, MIXED = 1, 5  # rows the tests look at by number


def candidate_rows(rng, indptr, indices):
    """70 rows.  0: empty; 1: of the user who has seen everything; 2: one candidate; 3, 4: the whole catalogue,
    shuffled; 5: a seen id, id 0, id I, a negative id and one id three times; then lengths k and k + 1 for every k
    under test, and 63 .. 65, T - 1 .. T + 1 and 2 T + 3 (drawn with replacement: duplicates); users repeat."""
    T = mod().RERANK_TILE
    users = rng.integers(0, U, N).astype(np.int32)
    users[:6] = [0, 1, 2, 0, 3, 5]
    rows = [rng.integers(1, I, rng.integers(0, 41)).astype(np.int32) for _ in range(N)]
    rows[0] = np.zeros(0, np.int32)
    rows[ALL_SEEN] = rng.integers(1, I, 20).astype(np.int32)
    rows[2] = np.array([128], np.int32)
    rows[3] = rng.permutation(np.arange(1, I)).astype(np.int32)
    rows[4] = rng.permutation(np.arange(1, I)).astype(np.int32)
    seen5 = indices[indptr[5]:indptr[6]]
    free5 = np.setdiff1d(np.arange(1, I), seen5)
    rows[MIXED] = np.array([free5[3], seen5[0], 0, free5[0], I, -7, free5[0], free5[1], free5[0]], np.int32)
    lengths = [1, 2, 10, 11, 128, 129, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
    for j, length in enumerate(lengths):
        rows[6 + j] = rng.integers(1, I, length).astype(np.int32)
    users[6 + len(lengths) - 1] = 0  # 2 T + 3 candidates, nothing seen: more than k + T live ones
    rows[N - 1] = rng.integers(1, I, T + 1).astype(np.int32)  # (in the partial last group)
    rows[N - 2] = rng.permutation(np.arange(1, I)).astype(np.int32)
    users[N - 2] = 2
    users[N - 3] = users[7]
    cptr, citems = csr_of(rows)
    return users, cptr, citems


@pytest.fixture(scope="module")
def exact():
    """Tables from {-4 .. 4} / 4 and biases from multiples of 1 / 4 (tests/test_gpu_rank.py::exact): every score is
    exact in fp32 in any order, and ties are plentiful.  The model's answers are computed once per (d, bias, csr), at
    k = 128: a smaller k is their first columns."""
    rng = np.random.default_rng(2025)
    indptr, indices = seen_csr(rng)
    users, cptr, citems = candidate_rows(rng, indptr, indices)
    cache = {}

    def case(d, bias, csr=True):
        key = (d, bias, csr)
        if key not in cache:
            g = np.random.default_rng(d)
            P = (g.integers(-4, 5, (U, d)) / 4).astype(np.float32)
            Q = (g.integers(-4, 5, (I, d)) / 4).astype(np.float32)
            b = (g.integers(-8, 9, I) / 4).astype(np.float32) if bias else None
            S = P.astype(np.float64) @ Q.T.astype(np.float64) + (b.astype(np.float64) if bias else 0.0)
            assert np.array_equal(S, S.astype(np.float32))
            want = rerank_rows(S.astype(np.float32), users, cptr, citems, 128,
                               *((indptr, indices) if csr else (None, None)))
            cache[key] = (P, Q, b, want)
        return cache[key]

    return dict(users=users, cptr=cptr, citems=citems, indptr=indptr, indices=indices, case=case)


@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(7)
    out = {}
    for d in (33, 128):
        P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
        out[d] = (P, Q, rng.standard_normal(I).astype(np.float32))
    out["csr"] = seen_csr(rng)
    out["rows"] = candidate_rows(rng, *out["csr"])
    return out


# ---- 4. exact against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", [8, 33, 128, 256])
def test_exact_against_the_model(exact, d, bias):
    users, cptr, citems = exact["users"], exact["cptr"], exact["citems"]
    for csr in (True, False):
        P, Q, b, want = exact["case"](d, bias, csr)
        ptr, idx = (exact["indptr"], exact["indices"]) if csr else (None, None)
        if csr:  # the data does hold what it is meant to
            assert (want[0][ALL_SEEN] == -1).all() and np.isneginf(want[2][cptr[ALL_SEEN]:cptr[ALL_SEEN + 1]]).all()
            five, dup = want[0][MIXED], citems[cptr[MIXED] + 3]
            at = np.flatnonzero(five == dup)
            assert len(at) == 3 and at[2] - at[0] == 2 and (five >= 0).sum() == 5  # three copies, adjacent
            assert np.isneginf(want[2][cptr[MIXED]:cptr[MIXED + 1]]).sum() == 4  # seen, 0, I, negative
            live = (want[0] >= 0).sum(1)
            assert (live < 1).any() and (live < 10).sum() > 5 and (live < 128).sum() > 20 and (live == 128).any()
            ties = sum(int((np.diff(s[i >= 0]) == 0).sum()) for i, s in zip(want[0], want[1]))
            assert ties > 100
        for layout in (0,) + mod().LAYOUTS:
            for k in KS:
                got = run(P, Q, b, users, cptr, citems, k, ptr, idx, layout=layout)
                w = (want[0][:, :k], want[1][:, :k], want[2])
                bad = np.flatnonzero((got[0] != w[0]).any(1) | (bits(got[1]) != bits(w[1])).any(1))
                assert same(got, w), (d, bias, csr, layout, k, bad[:8], got[0][bad[:2]], w[0][bad[:2]],
                                      np.flatnonzero(bits(got[2]) != bits(w[2]))[:8])


# ---- 5. the chain is recommend's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 128])
def test_full_lists_equal_recommend_bit_for_bit(floats, d):
    from revisit_bpr.recommend import recommend

    P, Q, b = floats[d]
    indptr, indices = floats["csr"]
    rng = np.random.default_rng(d)
    users = rng.integers(0, U, N).astype(np.int32)
    users[:4] = [0, 1, 2, 3]
    cptr, citems = csr_of([rng.permutation(np.arange(0, I)).astype(np.int32) for _ in range(N)])  # (id 0 too)
    for bias in (b, None):
        for ptr, idx in ((indptr, indices), (None, None)):
            for k in (10, 128):
                want = recommend(gpu(P), gpu(Q), gpu(bias), gpu(users), k, gpu(ptr), gpu(idx))
                want = tuple(o.cpu().numpy() for o in want)
                for layout in (0,) + mod().LAYOUTS:
                    got = run(P, Q, bias, users, cptr, citems, k, ptr, idx, layout=layout)
                    assert same(got[:2], want), (d, bias is not None, ptr is not None, k, layout)
    assert (want[0] >= 0).all() and len(np.unique(bits(want[1]))) > 1000  # (without the CSR: full rows, real floats)


# ---- 6. the chain is rank_items' ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 128])
def test_candidate_scores_equal_rank_items_bit_for_bit(floats, d):
    from revisit_bpr.ranks import rank_items

    P, Q, b = floats[d]
    indptr, indices = floats["csr"]
    users, cptr, citems = floats["rows"]
    for bias in (b, None):
        for ptr, idx in ((indptr, indices), (None, None)):
            want = rank_items(gpu(P), gpu(Q), gpu(bias), gpu(users), gpu(cptr), gpu(citems), gpu(ptr), gpu(idx))[2]
            want = want.cpu().numpy()
            for layout in (0,) + mod().LAYOUTS:
                got = mod().score_candidates(gpu(P), gpu(Q), gpu(bias), gpu(users), gpu(citems), gpu(cptr), gpu(ptr),
                                             gpu(idx), layout=layout).cpu().numpy()
                assert np.array_equal(bits(got), bits(want)), (d, bias is not None, ptr is not None, layout)
            if ptr is not None:
                assert 100 < np.isneginf(want).sum() < len(want) - 1000  # -inf where not eligible, on both sides


# ---- 7. a pure function of the inputs ----------------------------------------------------------------------------
def test_outputs_do_not_depend_on_order_split_or_layout(floats):
    P, Q, b = floats[128]
    indptr, indices = floats["csr"]
    users, cptr, citems = floats["rows"]
    rows = [citems[cptr[r]:cptr[r + 1]] for r in range(N)]
    rng = np.random.default_rng(11)
    for k in (10, 128):
        base = run(P, Q, b, users, cptr, citems, k, indptr, indices)
        for layout in mod().LAYOUTS:
            assert same(run(P, Q, b, users, cptr, citems, k, indptr, indices, layout=layout), base), layout
        # rows permuted
        perm = rng.permutation(N)
        p_ptr, p_items = csr_of([rows[r] for r in perm])
        got = run(P, Q, b, users[perm], p_ptr, p_items, k, indptr, indices)
        assert same(got[:2], (base[0][perm], base[1][perm]))
        assert same([got[2]], [np.concatenate([base[2][cptr[r]:cptr[r + 1]] for r in perm])])
        # candidates permuted inside their rows
        inner = [rng.permutation(len(r)) for r in rows]
        i_ptr, i_items = csr_of([r[p] for r, p in zip(rows, inner)])
        got = run(P, Q, b, users, i_ptr, i_items, k, indptr, indices)
        assert same(got[:2], base[:2])
        back = np.concatenate([got[2][cptr[r]:cptr[r + 1]][np.argsort(inner[r])] for r in range(N)])
        assert same([back], [base[2]])
        # the list twice
        t_ptr, t_items = csr_of(rows + rows)
        got = run(P, Q, b, np.concatenate([users, users]), t_ptr, t_items, k, indptr, indices)
        assert same(got, (np.concatenate([base[0]] * 2), np.concatenate([base[1]] * 2), np.concatenate([base[2]] * 2)))
        # the call in two
        cut = 37
        a_ptr, a_items = csr_of(rows[:cut])
        b_ptr, b_items = csr_of(rows[cut:])
        ga = run(P, Q, b, users[:cut], a_ptr, a_items, k, indptr, indices)
        gb = run(P, Q, b, users[cut:], b_ptr, b_items, k, indptr, indices)
        assert same(tuple(np.concatenate([x, y]) for x, y in zip(ga, gb)), base)


# ---- 8. the shared list ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 128])
def test_shared_list_equals_the_repeated_csr(floats, d):
    P, Q, b = floats[d]
    indptr, indices = floats["csr"]
    T = mod().RERANK_TILE
    rng = np.random.default_rng(3)
    L = rng.integers(1, I, 2 * T + 3).astype(np.int32)
    L[5], L[T], L[T + 7] = 0, L[3], I
    users = rng.integers(0, U, N).astype(np.int32)
    users[:3] = [0, 1, 2]
    rep = np.arange(N + 1, dtype=np.int64) * len(L)
    for k in (10, 128):
        want = run(P, Q, b, users, rep, np.tile(L, N), k, indptr, indices)
        for layout in (0,) + mod().LAYOUTS:
            got = run(P, Q, b, users, None, L, k, indptr, indices, layout=layout)
            assert same((got[0], got[1], got[2].reshape(-1)), want), (d, k, layout)
    short = L[:40]
    assert mod().layout_of(N, d, 10, len(short))[0] == mod().LAYOUT_WAVE  # (the plan's own choice, on a short list)
    got = run(P, Q, b, users, None, short, 10, indptr, indices)
    want = run(P, Q, b, users, np.arange(N + 1, dtype=np.int64) * 40, np.tile(short, N), 10, indptr, indices, layout=2)
    assert same((got[0], got[1], got[2].reshape(-1)), want)


def test_empty_calls():
    P, Q = torch.randn(U, 8).cuda(), torch.randn(I, 8).cuda()
    none32 = torch.zeros(0, dtype=torch.int32).cuda()
    users = torch.arange(3, dtype=torch.int32).cuda()
    it, sc, cs = mod().rerank(P, Q, None, none32, none32, 5, torch.zeros(1, dtype=torch.int64).cuda(), return_scores=True)
    assert it.shape == sc.shape == (0, 5) and cs.shape == (0,)
    for ptr in (torch.zeros(4, dtype=torch.int64).cuda(), None):  # three rows with no candidates, both forms
        it, sc, cs = mod().rerank(P, Q, None, users, none32, 5, ptr, return_scores=True)
        assert (it == -1).all() and torch.isneginf(sc).all() and cs.numel() == 0
        assert mod().score_candidates(P, Q, None, users, none32, ptr).numel() == 0
    with pytest.raises(ValueError, match="describe"):
        mod().rerank(P, Q, None, users, torch.ones(4, dtype=torch.int32).cuda(), 5,
                     torch.tensor([0, 2, 1, 4]).cuda())
    with pytest.raises(ValueError, match="describe"):
        mod().rerank(P, Q, None, users, torch.ones(4, dtype=torch.int32).cuda(), 5, torch.tensor([0, 1, 2, 3]).cuda())
    with pytest.raises(ValueError, match="out of range"):
        mod().rerank(P, Q, None, users + U - 2, torch.ones(4, dtype=torch.int32).cuda(), 5)


# ---- 9. no [nnz, d] buffer ---------------------------------------------------------------------------------------
def test_no_gathered_rows_buffer():
    n, C, k, d, Ub, Ib = 20_000, 1_000, 10, 128, 25_000, 20_109
    g = torch.Generator(device="cuda").manual_seed(1)
    P = torch.rand(Ub, d, device="cuda", generator=g)  # positive tables: a relative bound on a score means something
    Q = torch.rand(Ib, d, device="cuda", generator=g)
    b = torch.rand(Ib, device="cuda", generator=g)
    users = torch.randint(0, Ub, (n,), device="cuda", generator=g, dtype=torch.int32)
    cand = torch.randint(0, Ib, (n * C,), device="cuda", generator=g, dtype=torch.int32)
    cptr = torch.arange(n + 1, device="cuda", dtype=torch.int64) * C
    mod().rerank(P, Q, b, users[:8], cand[:8 * C], k, cptr[:9], return_scores=True)  # (the code is resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    items, scores, cs = mod().rerank(P, Q, b, users, cand, k, cptr, return_scores=True)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    outputs = n * k * 8 + n * C * 4
    print("growth", growth, "outputs", outputs, "gathered rows would be", n * C * d * 4)
    assert growth <= outputs + (1 << 20)
    pick = torch.randint(0, n, (64,), device="cuda", generator=g)
    ids = cand.view(n, C)[pick].long()
    ref = (Q[ids] * P[users[pick].long()][:, None]).sum(-1) + b[ids]
    ref = torch.where(ids > 0, ref, torch.full_like(ref, float("-inf")))
    got = cs.view(n, C)[pick]
    assert torch.equal(torch.isneginf(got), torch.isneginf(ref))
    live = ~torch.isneginf(ref)
    rel = ((got[live] - ref[live]).abs() / ref[live].abs()).max().item()
    print("largest relative difference of a score", rel)
    assert rel <= 1e-4
    top = torch.topk(ref, k, dim=1)
    assert ((scores[pick] - top.values).abs() <= 1e-4 * top.values.abs()).all()
    assert (items[pick] > 0).all()


# ---- 10. public layers -------------------------------------------------------------------------------------------
def test_engine_rerank_is_rerank_on_its_tables(floats):
    from revisit_bpr.engine import Engine

    P, Q, b = (gpu(x) for x in floats[128])
    tptr, tidx = (gpu(x) for x in floats["csr"])
    users, cptr, citems = (gpu(x) for x in floats["rows"])
    e = Engine(P, Q, b)
    none = e.rerank(users, citems, 20, cptr, return_scores=True)  # no CSR bound: nothing is seen
    assert all(torch.equal(x, y) for x, y in zip(none, mod().rerank(P, Q, b, users, citems, 20, cptr,
                                                                     return_scores=True)))
    e.bind_seen_csr(tptr, tidx)
    want = mod().rerank(P, Q, b, users, citems, 20, cptr, tptr, tidx, return_scores=True)
    got = e.rerank(users, citems, 20, cptr, return_scores=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and not torch.equal(got[0], none[0])
    assert torch.equal(e.score_candidates(users, citems, cptr), want[2])
    raw = e.rerank(users, citems, 20, cptr, exclude_seen=False, return_scores=True)
    assert all(torch.equal(x, y) for x, y in zip(raw, none))
    shared = e.rerank(users, citems[:50], 5)
    assert all(torch.equal(x, y) for x, y in zip(shared, mod().rerank(P, Q, b, users, citems[:50], 5, None, tptr, tidx)))
    assert torch.equal(e.score_candidates(users, citems[:50]),
                       mod().score_candidates(P, Q, b, users, citems[:50], None, tptr, tidx))
    e.close()


def small_model(Um, Im, d, user_bias):
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    torch.manual_seed(3)
    return BPR(fuse_forward=True, reg_alphas={"all": 0.001},
               logits_model=MF(torch.nn.Embedding(Um, d, padding_idx=0), torch.nn.Embedding(Im, d, padding_idx=0),
                               item_bias=True, user_bias=user_bias)).cuda()


@pytest.mark.parametrize("user_bias", [False, True])
def test_model_rerank_syncs_and_adds_the_user_bias(user_bias):
    """the stale-table check of tests/test_gpu_recommend.py"""
    from revisit_bpr import engine as eng
    from revisit_bpr.datasets import synthetic

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    model = small_model(data.num_users, data.num_items, 32, user_bias)
    if user_bias:
        with torch.no_grad():
            model.logits_model._user_bias.copy_(torch.randn(data.num_users, device="cuda"))
    tptr, tidx = gpu(data.indptr), gpu(data.indices)
    model.bind_seen_csr(tptr, tidx)
    g = torch.Generator(device="cuda").manual_seed(4)
    users = torch.arange(0, data.num_users, dtype=torch.int32, device="cuda")
    lens = torch.randint(0, 90, (users.numel(),), device="cuda", generator=g)
    cptr = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens, 0)])
    cand = torch.randint(0, data.num_items, (int(cptr[-1]),), device="cuda", generator=g, dtype=torch.int32)
    lm = model.logits_model

    def on_tables(exclude=True):
        sd = model.state_dict()
        it, sc, cs = mod().rerank(sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"],
                                  sd["logits_model._item_bias"], users, cand, 10, cptr, tptr if exclude else None,
                                  tidx if exclude else None, return_scores=True)
        if user_bias:
            ub = sd["logits_model._user_bias"][users.long()]
            sc, cs = sc + ub.unsqueeze(1), cs + torch.repeat_interleave(ub, lens)
        return it, sc, cs

    def equal(got, want):
        return all(torch.equal(x, y) for x, y in zip(got, want))

    assert equal(model.rerank(users, cand, 10, cptr, return_scores=True), on_tables())
    # a few Adam steps over small batches: rows touched early are behind the step count until replayed
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    tu, ti = gpu(data.users[:960].copy()), gpu(data.items[:960].copy())
    model.train_strict(opt, tu, ti, 64, eng.NEG_UNIFORM, seed=2)
    torch.cuda.synchronize()
    stale = lm._item_emb.weight.detach().clone()
    got = model.rerank(users, cand, 10, cptr, return_scores=True)  # must replay first ...
    assert not torch.equal(stale, lm._item_emb.weight.detach())  # (... and there was something to replay)
    want = on_tables()  # state_dict() syncs: the tables as they are at this step
    assert equal(got, want) and equal(model.rerank(users, cand, 10, cptr), want[:2])
    assert torch.equal(model.score_candidates(users, cand, cptr), want[2])
    raw = model.rerank(users, cand, 10, cptr, exclude_seen=False, return_scores=True)
    assert equal(raw, on_tables(exclude=False)) and not torch.equal(raw[0], got[0])
    # the shared list: the user bias goes to every column of a row
    L = cand[:70]
    it, sc, cs = model.rerank(users, L, 10, return_scores=True)
    sd = model.state_dict()
    w = mod().rerank(sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"],
                     sd["logits_model._item_bias"], users, L, 10, None, tptr, tidx, return_scores=True)
    ub = sd["logits_model._user_bias"][users.long()].unsqueeze(1) if user_bias else 0.0
    assert torch.equal(it, w[0]) and torch.equal(sc, w[1] + ub) and torch.equal(cs, w[2] + ub)
    assert torch.equal(model.score_candidates(users, L), cs)


def test_model_rerank_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        model.rerank(one, one, 3)
    with pytest.raises(NotImplementedError):
        model.score_candidates(one, one)
