"""The fused MMR kernel (`bpr_diversify_rows`, revisit-bpr_amd/csrc/bpr_diversify.hip) and what is built on it
(revisit_bpr.diversify.diversify / recommend_diverse, Engine and Model wrappers) on the GPU.

The yardstick is tests/diversify_model.py (brute force in numpy, pinned on the CPU by tests/test_diversify_cpu.py).
Contract under test (include/bprcore.h): a candidate is eligible iff 0 < id < I and its relevance is finite; the
similarity is k_topk's chain (cosine: dot * (rn(a) * rn(b))); each step picks the largest lam * rel' - oml * m, three
roundings, ties by larger relevance, smaller id, smaller position; the outputs are a pure function of the multiset
of (id, relevance) pairs of a row.

Shapes: a pool is padded to 32, 64, 96 or 128 candidates: C = 1, 31 .. 33, 64, 65, 127, 128 sit on both sides of
every cut and of the two waves that hold candidates; n = 70 rows is more than one workgroup; d = 33 takes the
element-load path and a padded chunk, d = 128 four chunks, d = 256 eight."""

import numpy as np
import pytest
import torch

from diversify_model import diversify_rows, sim_matrix

pytestmark = pytest.mark.gpu

U, I, N = 12, 300, 70
ZERO, TWIN_A, TWIN_B, TRIPLE = 17, 20, 21, 33  # a zero item row; two ids with one item row; the id listed three times
CS = (1, 31, 32, 33, 64, 65, 127, 128)
LAMS = (0.0, 0.5, 0.75, 1.0)
COMBOS = [(s, lam) for s in ("none", "minmax") for lam in LAMS]
_cache = {}


def mod():
    from revisit_bpr import diversify

    return diversify


def gpu(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()


def run(Q, ci, cs, k, layout=0, **kw):
    """(items, scores, mmr) as numpy"""
    out = mod().diversify(gpu(Q), gpu(ci), gpu(cs), k, return_mmr=True, layout=layout, **kw)
    torch.cuda.synchronize()
    assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.float32]
    assert out[0].shape == out[1].shape == out[2].shape == (len(ci), k)
    return tuple(o.cpu().numpy() for o in out)


def bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def int_table(d):
    """entries in [-3, 3]: every dot product is exact in fp32 whatever the order.  Computed once, never changed."""
    if ("Q", d) not in _cache:
        g = np.random.default_rng(d)
        Q = g.integers(-3, 4, (I, d)).astype(np.float32)
        Q[0] = 0
        Q[ZERO] = 0
        Q[TWIN_B] = Q[TWIN_A]
        Q.setflags(write=False)
        _cache["Q", d] = Q
    return _cache["Q", d]


def int_sims(d, metric):
    if ("S", d, metric) not in _cache:
        S = sim_matrix(int_table(d), metric)
        S.setflags(write=False)
        _cache["S", d, metric] = S
    return _cache["S", d, metric]


def pools(C, k, seed):
    """N rows of C candidates with dyadic relevances (so that ties in v are plentiful), the first rows special."""
    g = np.random.default_rng(1000 * C + k + seed)
    ci = g.integers(1, I, (N, C)).astype(np.int32)
    cs = (g.integers(-8, 9, (N, C)) / 4).astype(np.float32)

    def put(r, ids, rel):
        m = min(C, len(ids))
        ci[r, :m], cs[r, :m] = ids[:m], rel[:m]

    ci[0], cs[0] = -1, -np.inf                      # all padding (an empty pool)
    ci[1] = 0                                       # nothing eligible, by id
    ci[2], cs[2] = -1, -np.inf
    ci[2, C - 1], cs[2, C - 1] = 5, 0.25            # one candidate
    put(3, [0, I, -7, 9, 10, I - 1], [1, 1, 1, -np.inf, np.nan, 0.5])
    put(4, [TRIPLE] * 3, [1.5, 1.5, 1.5])           # an id three times, equal relevances ...
    put(5, [TRIPLE] * 3, [1.5, 0.5, 1.0])           # ... and unequal
    put(6, [TWIN_A, TWIN_B, ZERO], [1.0, 1.0, 2.0])  # identical item rows; a zero row
    put(7, [ZERO, TWIN_B, TWIN_A], [0.0, 0.5, 0.5])
    for r, cnt in ((8, k), (9, k - 1)):             # exactly k and k - 1 eligible candidates
        cnt = max(0, min(cnt, C))
        ci[r], cs[r] = -1, -np.inf
        ci[r, :cnt] = g.choice(np.arange(1, I), cnt, replace=False)
        cs[r, :cnt] = g.integers(-8, 9, cnt) / 4
    for r in range(10, 20):                         # what recommend returns for a short row: a padded tail
        cut = int(g.integers(0, C + 1))
        ci[r, cut:], cs[r, cut:] = -1, -np.inf
    return ci, cs


# ---- 1. exact on integer tables ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("d", [33, 128, 256])
def test_integer_tables_bit_for_bit(d, metric):
    """items, scores and mmr equal the model for every C and every k of {1, 10, C, 128}; each (C, k) runs two of the
    eight (scale, lam) pairs, in rotation, so that every pair meets every C"""
    Q, S = int_table(d), int_sims(d, metric)
    assert np.array_equal(S, S.T)
    ties, seen, idx = 0, set(), 0
    for C in CS:
        for k in sorted({1, 10, C, 128}):
            ci, cs = pools(C, k, d)
            for scale, lam in (COMBOS[idx % 8], COMBOS[(idx + 5) % 8]):
                want = diversify_rows(S, ci, cs, k, lam, scale)
                got = run(Q, ci, cs, k, lam=lam, metric=metric, scale=scale)
                assert np.array_equal(got[0], want[0]), (C, k, scale, lam)
                assert np.array_equal(bits(got[1]), bits(want[1])), (C, k, scale, lam)
                assert np.array_equal(got[2], want[2]), (C, k, scale, lam)  # (as values: -0 is 0)
                ties += want[3]
                seen.add((scale, lam))
            idx += 1
            assert (want[0][:3] == -1).sum() >= 3 * k - 1 and want[0][2, 0] in (5, -1)
    assert seen == set(COMBOS)
    print("steps decided by the tie rule:", ties)
    assert ties > 100  # the cases do contain exact ties in v


# ---- 2. the chain is k_topk's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 128, 256])
def test_second_pick_carries_the_score_kernels_bits(d):
    """float tables, dot, lam = 0, k = 2: the second pick's v is -(its similarity to the first), the largest such:
    bitwise the negated minimum of what score_candidates returns for (first pick, the row's other candidates)"""
    from revisit_bpr.rerank import score_candidates

    C = 100
    g = np.random.default_rng(d)
    Q = (g.standard_normal((I, d)) * 0.1).astype(np.float32)
    ci = np.stack([g.choice(np.arange(1, I), C, replace=False) for _ in range(N)]).astype(np.int32)
    cs = g.standard_normal((N, C)).astype(np.float32)
    items, scores, mmr = run(Q, ci, cs, 2, lam=0.0, metric="dot")
    first = items[:, 0]
    assert np.array_equal(first, ci[np.arange(N), cs.argmax(1)])  # v ties at 0: the most relevant
    cptr = np.arange(N + 1, dtype=np.int64) * C
    Qg = gpu(Q)
    sc = score_candidates(Qg, Qg, None, gpu(first), gpu(ci.reshape(-1)), gpu(cptr)).cpu().numpy().reshape(N, C)
    sc[ci == first[:, None]] = np.inf
    want = (-sc.min(1)).astype(np.float32)
    assert np.array_equal(bits(mmr[:, 1]), bits(want))
    assert np.array_equal(items[:, 1], ci[np.arange(N), sc.argmin(1)])


# ---- 3. float tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["none", "minmax"])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("d", [33, 128])
def test_float_tables_greedy_within_the_fp32_bound(d, metric, scale):
    """For every returned pick p, v recomputed in float64 for every still-unpicked candidate c given the picks before
    it: v64(p) + eps(p) >= v64(c) - eps(c).  u = 2^-24; eps from d and the magnitudes, to first order with slack:
      sim, dot:     d u sum_f |a_f b_f| (the standard bound of an fp32 chain of length d; staged zeros add nothing);
      sim, cosine:  u (d sum_f |a_f b_f| / (|a| |b|) + (d + 8) |S|) — tests/test_gpu_similar.py's derivation: rn(v) is
                    within (d / 2 + 2) u of 1 / |v|, two of them, two multiplications (here rn(a) rn(b) first, the
                    count is the same), 2 u |S| of slack;
      m:            a maximum moves by at most the largest error of its terms: eps_m(c) = max over picked s;
      rel':         exact (none), or three roundings of a value in [0, 1]: 4 u |rel'| (minmax);
      v:            lam rel' rounds once (u), oml = 1 - lam rounds once and oml m once (2 u oml |m|), the
                    subtraction once (u |v|): eps = lam (4 u |rel'| [minmax] + u |rel'|) + oml (eps_m + 2 u |m|) +
                    2 u |v|.
    Every row is checked; pools are drawn without replacement from N(0, 0.1) tables."""
    C, k, lam = 100, 10, 0.7
    g = np.random.default_rng(7 * d + len(metric) + len(scale))
    Q = (g.standard_normal((I, d)) * 0.1).astype(np.float32)
    ci = np.stack([g.choice(np.arange(1, I), C, replace=False) for _ in range(N)]).astype(np.int32)
    cs = g.standard_normal((N, C)).astype(np.float32)
    items, scores, mmr = run(Q, ci, cs, k, lam=lam, metric=metric, scale=scale)
    u = 2.0 ** -24
    Q64 = Q.astype(np.float64)
    X = Q64[ci]                                                   # [N, C, d]: float64 on the host, the reference
    G = np.einsum("ncd,ned->nce", X, X)
    mag = np.einsum("ncd,ned->nce", np.abs(X), np.abs(X))
    if metric == "cosine":
        nrm = np.sqrt((X ** 2).sum(-1))
        den = nrm[:, :, None] * nrm[:, None, :]
        Sim = G / den
        eps_sim = u * (d * mag / den + (d + 8) * np.abs(Sim))
    else:
        Sim, eps_sim = G, d * u * mag
    rel = cs.astype(np.float64)
    relp = rel
    if scale == "minmax":
        lo, hi = rel.min(1, keepdims=True), rel.max(1, keepdims=True)
        relp = (rel - lo) / (hi - lo)
    lam32 = float(np.float32(lam))
    oml = float(np.float32(1) - np.float32(lam))
    rows = np.arange(N)
    left = np.ones((N, C), bool)
    m = np.zeros((N, C))
    eps_m = np.zeros((N, C))
    worst = -np.inf
    for step in range(k):
        pos = (ci == items[:, step][:, None]).argmax(1)
        assert (ci[rows, pos] == items[:, step]).all() and left[rows, pos].all()  # a candidate, not picked before
        assert np.array_equal(bits(scores[:, step]), bits(cs[rows, pos]))
        v = lam32 * relp - oml * m
        eps = lam32 * (5 if scale == "minmax" else 1) * u * np.abs(relp) + oml * (eps_m + 2 * u * np.abs(m)) \
            + 2 * u * np.abs(v)
        upper = (v + eps)[rows, pos]
        lower = np.where(left, v - eps, -np.inf).max(1)
        worst = max(worst, float((lower - upper).max()))
        assert (upper >= lower).all(), (step, float((lower - upper).max()))
        assert (np.abs(mmr[:, step] - v[rows, pos]) <= eps[rows, pos] + u * np.abs(v[rows, pos])).all()
        left[rows, pos] = False
        s, e = Sim[rows, :, pos], eps_sim[rows, :, pos]
        m, eps_m = (s, e) if step == 0 else (np.maximum(m, s), np.maximum(eps_m, e))
    print("largest (best left out - eps) - (picked + eps):", worst)


# ---- 4. links to the rest ----------------------------------------------------------------------------------------
def test_lam_one_is_the_sorted_pool_and_recommend():
    from revisit_bpr.recommend import recommend

    Q = int_table(128)
    ci, cs = pools(100, 100, 4)
    got = run(Q, ci, cs, 100, lam=1.0, metric="cosine", scale="none")
    for r in range(N):
        pool = sorted((-float(s), int(i)) for i, s in zip(ci[r], cs[r]) if 0 < i < I and np.isfinite(s))
        assert got[0][r, :len(pool)].tolist() == [p[1] for p in pool] and (got[0][r, len(pool):] == -1).all()
        assert got[1][r, :len(pool)].tolist() == [-p[0] for p in pool]
    # recommend_diverse(lam = 1) is recommend(k), with a seen CSR (user 1 has seen everything, user 2 nearly)
    g = np.random.default_rng(8)
    P = ((g.random((U, 128)) - 0.5) / 8).astype(np.float32)
    Qf = ((g.random((I, 128)) - 0.5) / 8).astype(np.float32)
    b = (g.random(I) * 0.01).astype(np.float32)
    seen = [np.flatnonzero(g.random(I - 1) < 0.3).astype(np.int32) + 1 for _ in range(U)]
    seen[1] = np.arange(1, I, dtype=np.int32)
    seen[2] = np.arange(1, I - 40, dtype=np.int32)
    indptr = gpu(np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64))
    indices = gpu(np.concatenate(seen).astype(np.int32))
    users = gpu(np.arange(U, dtype=np.int32))
    Pg, Qg, bg = gpu(P), gpu(Qf), gpu(b)
    want = recommend(Pg, Qg, bg, users, 10, indptr, indices)
    for scale in ("minmax", "none"):
        got = mod().recommend_diverse(Pg, Qg, bg, users, 10, pool=100, lam=1.0, scale=scale, seen_indptr=indptr,
                                      seen_indices=indices)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert (want[0][1] == -1).all() and (want[0][2] >= 0).all()


def test_diversifying_does_not_raise_intra_list_similarity():
    """cosine, top 10 of 100 on the integer fixture: the model's lists at lam < 1 are, on average, no more alike than
    at lam = 1 (computed exactly by the model first); the kernel returns those lists"""
    Q, S = int_table(128), int_sims(128, "cosine")
    ci, cs = pools(100, 10, 5)

    def ils(items):
        out = []
        for row in items:
            ids = row[row >= 0]
            if len(ids) > 1:
                sub = S[np.ix_(ids, ids)].astype(np.float64)
                out.append((sub.sum() - np.trace(sub)) / (len(ids) * (len(ids) - 1)))
            else:
                out.append(0.0)
        return np.array(out)

    base = diversify_rows(S, ci, cs, 10, 1.0, "minmax")[0]
    for lam in (0.75, 0.5, 0.0):
        want = diversify_rows(S, ci, cs, 10, lam, "minmax")[0]
        assert ils(want).mean() <= ils(base).mean()
        got = run(Q, ci, cs, 10, lam=lam, metric="cosine", scale="minmax")[0]
        assert np.array_equal(got, want)
        mine = mod().intra_list_similarity(gpu(Q), gpu(got)).cpu().numpy()
        assert np.allclose(mine, ils(want), atol=1e-5)
        assert mine.mean() <= ils(base).mean() + 1e-6


# ---- 5. a pure function of the inputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("C, k", [(32, 10), (100, 10), (128, 128)])
def test_pure_function_of_the_inputs(C, k):
    g = np.random.default_rng(C + k)
    Q = (g.standard_normal((I, 128)) * 0.1).astype(np.float32)
    Q[TWIN_B] = Q[TWIN_A]
    ci, cs = pools(C, k, 6)
    cs = (cs + g.integers(0, 2, cs.shape) * g.standard_normal(cs.shape) * 0.01).astype(np.float32)
    for metric, scale in (("cosine", "minmax"), ("dot", "none")):
        kw = dict(lam=0.5, metric=metric, scale=scale)
        base = run(Q, ci, cs, k, **kw)
        perm = g.permutation(N)                               # the rows in another order
        got = run(Q, ci[perm], cs[perm], k, **kw)
        assert same(got, tuple(x[perm] for x in base))
        inner = g.permuted(np.tile(np.arange(C), (N, 1)), axis=1)  # the candidates inside every row
        assert same(run(Q, np.take_along_axis(ci, inner, 1), np.take_along_axis(cs, inner, 1), k, **kw), base)
        parts = [run(Q, ci[a:b], cs[a:b], k, **kw) for a, b in ((0, 1), (1, 37), (37, N))]  # the call split
        assert same(tuple(np.concatenate(x) for x in zip(*parts)), base)
        for layout in (0,) + mod().LAYOUTS:
            assert same(run(Q, ci, cs, k, layout=layout, **kw), base)
        one = mod().diversify(gpu(Q), gpu(ci[11]), gpu(cs[11]), k, **kw)  # a 1-D row
        assert one[0].shape == (k,) and np.array_equal(one[0].cpu().numpy(), base[0][11])


def test_outputs_of_recommend_and_rerank_go_in_unchanged():
    from revisit_bpr.recommend import recommend
    from revisit_bpr.rerank import rerank

    g = np.random.default_rng(9)
    P = gpu((g.standard_normal((U, 64)) * 0.1).astype(np.float32))
    Q = gpu((g.standard_normal((I, 64)) * 0.1).astype(np.float32))
    seen = [np.arange(1, I - 7 * u, dtype=np.int32) for u in range(U)]  # user u has 7 u unseen items left
    indptr = gpu(np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64))
    indices = gpu(np.concatenate(seen).astype(np.int32))
    users = gpu(np.arange(U, dtype=np.int32))
    cand, rel = recommend(P, Q, None, users, 50, indptr, indices)
    assert (cand[0] == -1).all() and (cand[3] == -1).sum() == 50 - 21 and (cand[8] >= 0).all()
    got = mod().diversify(Q, cand, rel, 10, lam=0.0, metric="dot")
    assert (got[0][0] == -1).all() and torch.isneginf(got[1][0]).all() and (got[0][1] >= 0).sum() == 7
    for r in range(U):  # every pick is one of the row's candidates with its own score, none twice
        live = got[0][r][got[0][r] >= 0].tolist()
        assert len(set(live)) == len(live) == min(10, 7 * r)
        lookup = dict(zip(cand[r].tolist(), rel[r].tolist()))
        assert [lookup[i] for i in live] == got[1][r][: len(live)].tolist()
    pool = gpu(g.integers(-1, I + 1, 90).astype(np.int32))
    cand2, rel2 = rerank(P, Q, None, users, pool, 64, seen_indptr=indptr, seen_indices=indices)
    got2 = mod().diversify(Q, cand2, rel2, 64, lam=1.0)
    assert torch.equal(got2[0], cand2) and torch.equal(got2[1].view(torch.int32), rel2.view(torch.int32))


# ---- 6. wrappers -------------------------------------------------------------------------------------------------
def small_model(nu, ni, d):
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    torch.manual_seed(3)
    return BPR(fuse_forward=True, reg_alphas={"all": 0.001},
               logits_model=MF(torch.nn.Embedding(nu, d, padding_idx=0), torch.nn.Embedding(ni, d, padding_idx=0),
                               item_bias=True, user_bias=False)).cuda()


def test_engine_and_model_equal_the_module_function():
    from revisit_bpr import engine as eng
    from revisit_bpr.datasets import synthetic

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    model = small_model(data.num_users, data.num_items, 32)
    model.bind_seen_csr(gpu(data.indptr), gpu(data.indices))
    users = torch.arange(1, 60, dtype=torch.int32, device="cuda")

    def same_t(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def on_tables():
        sd = model.state_dict()  # syncs: the tables as they are at this step
        P, Q = sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"]
        bias = sd["logits_model._item_bias"].reshape(-1)
        want = mod().recommend_diverse(P, Q, bias, users, 10, pool=50, lam=0.5, seen_indptr=gpu(data.indptr),
                                       seen_indices=gpu(data.indices))
        return Q, want

    Q, want = on_tables()
    e = model.engine()
    assert same_t(e.recommend_diverse(users, 10, pool=50, lam=0.5), want)
    assert same_t(model.recommend_diverse(users, 10, pool=50, lam=0.5), want)
    cand, rel = model.recommend(users, 50)
    for kw in (dict(lam=0.3, metric="dot", return_mmr=True), dict(scale="minmax")):
        w = mod().diversify(Q, cand, rel, 7, **kw)
        assert same_t(e.diversify(cand, rel, 7, **kw), w) and same_t(model.diversify(cand, rel, 7, **kw), w)
    # a few Adam steps over small batches: rows touched early are behind the step count until replayed
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    tu, ti = gpu(data.users[:960].copy()), gpu(data.items[:960].copy())
    model.train_strict(opt, tu, ti, 64, eng.NEG_UNIFORM, seed=2)
    torch.cuda.synchronize()
    stale = model.logits_model._item_emb.weight.detach().clone()
    got = model.diversify(cand, rel, 7, lam=0.3, metric="dot", return_mmr=True)  # must replay first ...
    assert not torch.equal(stale, model.logits_model._item_emb.weight.detach())  # (... there was something to replay)
    Q, want = on_tables()
    assert same_t(got, mod().diversify(Q, cand, rel, 7, lam=0.3, metric="dot", return_mmr=True))
    assert not same_t(got, mod().diversify(stale, cand, rel, 7, lam=0.3, metric="dot", return_mmr=True))
    assert same_t(model.recommend_diverse(users, 10, pool=50, lam=0.5), want)


def test_model_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    ci, cs = torch.ones(1, 4, dtype=torch.int32, device="cuda"), torch.zeros(1, 4, device="cuda")
    with pytest.raises(NotImplementedError):
        model.diversify(ci, cs, 3)
    with pytest.raises(NotImplementedError):
        model.recommend_diverse(torch.ones(1, dtype=torch.int32, device="cuda"), 3)


# ---- 7. no [n, C, C] and no [n, C, d] buffer ---------------------------------------------------------------------
def test_no_gather_and_no_similarity_buffer():
    n, C, d, k = 20_000, 128, 128, 20
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = (torch.rand(20_109, d, device="cuda", generator=g) - 0.5) / d
    ci = torch.randint(1, 20_109, (n, C), device="cuda", generator=g, dtype=torch.int32)
    cs = torch.rand(n, C, device="cuda", generator=g)
    mod().diversify(Q, ci[:64], cs[:64], k)  # (the library is loaded, the kernel's code is resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    items, scores, mmr = mod().diversify(Q, ci, cs, k, return_mmr=True)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    outputs = n * k * 12
    print("peak growth", growth, "outputs", outputs, "either buffer would be", n * C * C * 4)
    assert growth <= outputs + (64 << 20) < n * C * C * 4 // 15
    it = items.cpu().numpy()
    assert (it >= 1).all()
    ci_np, cs_np, sc = ci.cpu().numpy(), cs.cpu().numpy(), scores.cpu().numpy()
    # every pick is one of its row's (id, relevance) pairs (an id may be listed twice in a row of random ids)
    assert ((ci_np[:, :, None] == it[:, None, :]) & (cs_np[:, :, None] == sc[:, None, :])).any(1).all()
    assert np.array_equal(sc[:, 0], cs_np.max(1))  # the first pick is the most relevant


# ---- 8. captured in a graph --------------------------------------------------------------------------------------
def test_captured_in_a_graph_replays_the_same_bits():
    """one linear capture (a single kernel on the capturing stream, no parallel branches), replayed twice"""
    g = np.random.default_rng(11)
    Q = gpu((g.standard_normal((I, 128)) * 0.1).astype(np.float32))
    ci_np, cs_np = pools(100, 10, 7)
    ci, cs = gpu(ci_np), gpu(cs_np)
    kw = dict(lam=0.7, metric="cosine", scale="minmax", return_mmr=True)
    eager = [t.clone() for t in mod().diversify(Q, ci, cs, 10, **kw)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mod().diversify(Q, ci, cs, 10, **kw)
    for _ in range(2):
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, eager))
    ci2, cs2 = pools(100, 10, 8)  # the graph reads its inputs where they are: new pools, same addresses
    ci.copy_(gpu(ci2))
    cs.copy_(gpu(cs2))
    graph.replay()
    torch.cuda.synchronize()
    want = mod().diversify(Q, ci, cs, 10, **kw)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, want))
