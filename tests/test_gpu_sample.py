"""`bpr_sample_rows` (revisit-bpr_amd/csrc/bpr_sample.hip, revisit_bpr/sample.py) on the GPU: k unseen items per user
drawn without replacement from softmax(score / T), held to the host model tests/sample_model.py bit for bit — items,
keys and scores; there is no tolerance on them anywhere.  What the model is worth is measured on the CPU
(tests/test_sample_model_cpu.py: its logarithm against float64 over every uniform, its draws against the
Plackett-Luce distribution); the 200,000-row case of that file is run here as one call and compared bit for bit, which
takes its statistics over without repeating them.  log_z alone is held to a tolerance, derived below.

Shapes are the smallest that cover every path: I = 300 (two full item tiles and one of 44), n = 70 rows (a full user
tile and one of 6), d = 20 (element loads), 32 (one chunk), 40 (two chunks with a tail), k = 1, 10, 128, with and
without bias, item_slices 1 and 3, T = 0.25, 1, 4, and a seen CSR in which user 1 has seen all but 3 items."""
import functools

import numpy as np
import pytest
import torch

import sample_model as sm
from chain_model import F, bits, chain_scores

pytestmark = pytest.mark.gpu

U, I, N_ROWS = 48, 300, 70
CASES = [(d, bias, T) for d in (20, 32, 40) for bias in (False, True) for T in (0.25, 1.0, 4.0)]
CASE_IDS = [f"d{d}-{'bias' if bias else 'nobias'}-T{T}" for d, bias, T in CASES]
SEED = 0x5EED0123456789AB  # (both key words in use)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_csr(rng, n_users=U, n_items=I):
    """int64 [U+1], int32 sorted per row, items 1 .. I-1: user 0 has seen nothing, user 1 everything but 3 items,
    user 2 everything, the rest a random fifth"""
    rows = []
    for u in range(n_users):
        if u == 0:
            rows.append(np.zeros(0, np.int32))
        elif u == 1:
            keep = rng.choice(np.arange(1, n_items), size=3, replace=False)
            rows.append(np.setdiff1d(np.arange(1, n_items), keep).astype(np.int32))
        elif u == 2:
            rows.append(np.arange(1, n_items, dtype=np.int32))
        else:
            rows.append(np.flatnonzero(rng.random(n_items - 1) < 0.2).astype(np.int32) + 1)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(d, bias, T):
    """inputs of one (d, bias, T) and the model's result at k = 128, computed once and never changed: the model's
    result at a smaller k is its prefix (the order is total)"""
    rng = np.random.default_rng(1000 * d + 10 * int(bias) + int(4 * T))
    c = Case()
    c.P, c.Q = rng.standard_normal((U, d)).astype(F), rng.standard_normal((I, d)).astype(F)
    c.b = rng.standard_normal(I).astype(F) if bias else None
    c.indptr, c.indices = make_csr(rng)
    c.users = np.concatenate([np.arange(U), rng.integers(0, U, N_ROWS - U)]).astype(np.int32)
    rng.shuffle(c.users)
    # T = 1 runs on the default draw id, the user; the others on ids of their own, negative ones and > 2^32 among them
    c.draw_ids = None if T == 1.0 else rng.integers(-2 ** 62, 2 ** 62, N_ROWS).astype(np.int64)
    c.T = T
    c.items, c.scores, c.keys, c.S = sm.sample_rows(c.P, c.Q, c.b, c.users, 128, c.indptr, c.indices, T, SEED,
                                                    c.draw_ids)
    c.t = [dev(x) for x in (c.P, c.Q, c.b)]
    c.csr = (dev(c.indptr), dev(c.indices))
    return c


def run(c, k, rows=None, **kw):
    from revisit_bpr.sample import sample_items

    rows = np.arange(len(c.users)) if rows is None else np.asarray(rows)
    did = None if c.draw_ids is None else dev(c.draw_ids[rows])
    kw.setdefault("temperature", c.T)
    kw.setdefault("seed", SEED)
    out = sample_items(*c.t, dev(c.users[rows]), k, *c.csr, draw_ids=did, return_keys=True, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. bits against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, bias, T", CASES, ids=CASE_IDS)
def test_items_keys_and_scores_are_the_models_bits(d, bias, T):
    c = case(d, bias, T)
    for k in (1, 10, 128):
        for item_slices in (1, 3):
            items, scores, keys = run(c, k, item_slices=item_slices)
            what = f"k={k} slices={item_slices}"
            assert np.array_equal(items, c.items[:, :k]), what
            assert same_bits(keys, c.keys[:, :k]), what
            assert same_bits(scores, c.scores[:, :k]), what


# ---- 2. purity --------------------------------------------------------------------------------------------------------
def test_result_is_a_function_of_the_row_alone():
    c = case(40, True, 0.25)
    base = run(c, 10, item_slices=1)
    perm = np.random.default_rng(7).permutation(N_ROWS)
    got = run(c, 10, rows=perm, item_slices=1)
    for g, b in zip(got, base):
        assert same_bits(g, b[perm])
    for r in (0, 37, 69):  # n = 1 against the same row inside n = 70
        for g, b in zip(run(c, 10, rows=[r], item_slices=1), base):
            assert same_bits(g[0], b[r])
    for item_slices in (3, 0):
        for g, b in zip(run(c, 10, item_slices=item_slices), base):
            assert same_bits(g, b)


def test_draw_id_decides_the_draw():
    from revisit_bpr.sample import sample_items

    c = case(32, False, 1.0)
    users = dev(np.array([5, 5, 5], np.int32))
    did = np.array([11, 11, 12], np.int64)
    want = sm.sample_rows(c.P, c.Q, None, [5, 5, 5], 10, c.indptr, c.indices, 1.0, 3, did)[0]
    assert np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2])  # the model says they differ
    items, scores, keys = sample_items(*c.t, users, 10, *c.csr, seed=3, draw_ids=dev(did), return_keys=True)
    items = items.cpu().numpy()
    assert np.array_equal(items, want)
    assert torch.equal(keys[0], keys[1]) and torch.equal(scores[0], scores[1])
    assert not np.array_equal(items[0], items[2])
    # another seed is another draw
    other = sample_items(*c.t, users, 10, *c.csr, seed=4, draw_ids=dev(did))[0].cpu().numpy()
    assert np.array_equal(other, sm.sample_rows(c.P, c.Q, None, [5, 5, 5], 10, c.indptr, c.indices, 1.0, 4, did)[0])
    assert not np.array_equal(other, items)


# ---- 3. the scores are score_candidates' ------------------------------------------------------------------------------
@pytest.mark.parametrize("d, bias", [(20, True), (40, False)])
def test_scores_equal_score_candidates(d, bias):
    from revisit_bpr.rerank import score_candidates

    c = case(d, bias, 4.0)
    from revisit_bpr.sample import sample_items

    users = dev(c.users)
    items, scores = sample_items(*c.t, users, 128, *c.csr, temperature=4.0, seed=SEED, draw_ids=dev(c.draw_ids))
    indptr = torch.arange(N_ROWS + 1, dtype=torch.int64, device="cuda") * 128
    want = score_candidates(*c.t, users, items.reshape(-1), indptr, *c.csr).reshape(N_ROWS, 128)
    assert same_bits(scores.cpu().numpy(), want.cpu().numpy())
    assert (items >= 0).sum() > 100 * N_ROWS // 2


# ---- 4. eligibility ---------------------------------------------------------------------------------------------------
def test_eligibility_padding_nan_and_inf():
    from revisit_bpr.sample import sample_items

    c = case(32, True, 1.0)
    J_NAN, J_INF = 77, 201
    Q = c.Q.copy()
    Q[J_NAN] = np.nan
    b = c.b.copy()
    b[J_INF] = np.inf
    users = dev(c.users)
    for item_slices in (1, 3):
        items, scores, keys = sample_items(dev(c.P), dev(Q), dev(b), users, 128, *c.csr, seed=SEED, return_keys=True,
                                           item_slices=item_slices)
        items, scores, keys = items.cpu().numpy(), scores.cpu().numpy(), keys.cpu().numpy()
        want = sm.sample_rows(c.P, Q, b, c.users, 128, c.indptr, c.indices, 1.0, SEED)
        assert np.array_equal(items, want[0]) and same_bits(keys, want[2]) and same_bits(scores, want[1])
        for r, u in enumerate(c.users):
            seen = set(c.indices[c.indptr[u]:c.indptr[u + 1]].tolist())
            got = items[r][items[r] >= 0]
            assert 0 not in got and J_NAN not in got and not seen & set(got.tolist())
            assert len(set(got.tolist())) == len(got)                       # no id twice
            n_el = I - 1 - len(seen) - (J_NAN not in seen)
            assert len(got) == min(128, n_el)                               # everything eligible is drawn before padding
            assert np.all(items[r][len(got):] == -1)                        # the short row ends in -1 / -inf / -inf
            assert np.all(scores[r][len(got):] == -np.inf) and np.all(keys[r][len(got):] == -np.inf)
            assert np.all(keys[r][:-1] >= keys[r][1:])                      # draw order: key descending
            if J_INF not in seen:
                assert items[r][0] == J_INF and scores[r][0] == np.inf      # a +inf score is drawn first
        assert (items[c.users == 1] >= 0).sum(axis=1).max() <= 3 and np.all(items[c.users == 2] == -1)


# ---- 5. log_z ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, bias, T", [(20, True, 0.25), (40, False, 1.0), (32, True, 4.0)])
def test_log_z_against_float64(d, bias, T):
    """log_z against float64 on the host from numpy scores (chain_model, independent of `recommend`); inputs scaled so
    that |score / T| <= 8.  Bound on the absolute error: (I + 32) * 2^-23 — the recursive fp32 summation of I positive
    terms gives at most (I - 1) * 2^-24 relative on the sum, hence absolute on its logarithm; the rest covers the
    rounding of the exponent's argument (|x - m| <= 16: 2^-20 relative per term at most before the exp) and the two
    intrinsics.  Equal bits when the call is repeated; -inf for the user who has seen everything."""
    from revisit_bpr.sample import sample_items

    c = case(d, bias, T)
    S = chain_scores(c.P[c.users], c.Q, c.b)
    scale = F(min(1.0, 7.9 * T / np.abs(S).max()))
    P = (c.P * scale).astype(F)
    b = None if c.b is None else (c.b * scale).astype(F)
    S = chain_scores(P[c.users], c.Q, b)
    inv_t = sm.inv_temperature(T)
    assert np.abs(S.astype(np.float64) * float(inv_t)).max() <= 8
    ok = sm.eligible(I, c.users, c.indptr, c.indices)
    want = sm.log_z64(S, ok, inv_t)
    bound = (I + 32) * 2.0 ** -23
    users = dev(c.users)
    for item_slices in (1, 3):
        def call():
            out = sample_items(dev(P), c.t[1], dev(b), users, 10, *c.csr, temperature=T, seed=SEED,
                               return_log_z=True, item_slices=item_slices)
            return out[0].cpu().numpy(), out[2].cpu().numpy()
        items, log_z = call()
        assert np.array_equal(log_z[c.users == 2], np.full((c.users == 2).sum(), -np.inf, F))
        live = c.users != 2
        err = np.abs(log_z[live].astype(np.float64) - want[live])
        print(f"slices={item_slices}: largest |log_z - float64| = {err.max():.3e}, bound {bound:.3e}")
        assert err.max() <= bound
        again = call()
        assert same_bits(again[1], log_z) and np.array_equal(again[0], items)
        # asking for log_z changes nothing else
        plain = sample_items(dev(P), c.t[1], dev(b), users, 10, *c.csr, temperature=T, seed=SEED,
                             item_slices=item_slices)[0].cpu().numpy()
        assert np.array_equal(plain, items)


def test_log_z_of_an_infinite_score_is_infinite():
    from revisit_bpr.sample import sample_items

    c = case(32, True, 1.0)
    b = c.b.copy()
    b[201] = np.inf
    log_z = sample_items(c.t[0], c.t[1], dev(b), dev(c.users), 3, *c.csr, return_log_z=True)[2].cpu().numpy()
    for r, u in enumerate(c.users):
        seen = c.indices[c.indptr[u]:c.indptr[u + 1]]
        assert (log_z[r] == np.inf) == (201 not in seen)
        assert not np.isnan(log_z[r])


def test_propensities_of_a_small_catalogue_sum_to_one():
    """an 8-item catalogue: k = 8 returns every item with its score, and exp(log_propensity) of the k = 1 outcomes —
    each item at position 0 — sums to 1 to 1e-5"""
    from revisit_bpr.sample import log_propensity, sample_items
    from test_sample_model_cpu import distribution_tables

    P, Q = distribution_tables()
    for T in (0.5, 1.0, 3.0):
        items, scores, log_z = sample_items(dev(P), dev(Q), None, dev(np.zeros(4, np.int32)), 8, temperature=T, seed=1,
                                            draw_ids=dev(np.arange(4, dtype=np.int64)), return_log_z=True)
        assert sorted(items[0].tolist()) == list(range(1, 9))
        first = log_propensity(scores.reshape(-1, 1), log_z.repeat_interleave(8), T).reshape(4, 8)
        assert torch.allclose(torch.exp(first).sum(dim=1), torch.ones(4, dtype=torch.float64, device="cuda"),
                              rtol=0, atol=1e-5)
        # and along a row the prefix probabilities multiply up to that of the whole permutation: finite, <= 0
        whole = log_propensity(scores, log_z, T).sum(dim=1)
        assert torch.isfinite(whole).all() and (whole <= 0).all()


# ---- 6. the distribution on the device --------------------------------------------------------------------------------
def test_two_hundred_thousand_rows_are_the_models():
    """The I = 9 case of tests/test_sample_model_cpu.py (200,000 rows, draw_ids = arange, its seed) in one call: the
    first two draws and their keys are the model's, bit for bit, so its chi-square statistics are the device's."""
    from revisit_bpr.sample import sample_items
    from test_sample_model_cpu import DIST_ROWS, DIST_SEED, distribution_draws, distribution_tables

    P, Q = distribution_tables()
    order, _ = distribution_draws()
    users = torch.zeros(DIST_ROWS, dtype=torch.int32, device="cuda")
    did = torch.arange(DIST_ROWS, dtype=torch.int64, device="cuda")
    items, scores, keys = sample_items(dev(P), dev(Q), None, users, 2, seed=DIST_SEED, draw_ids=did, return_keys=True)
    assert np.array_equal(items.cpu().numpy(), order.astype(np.int32))
    K = sm.keys(np.broadcast_to(chain_scores(P, Q), (DIST_ROWS, 9)), sm.inv_temperature(1.0), np.arange(DIST_ROWS),
                np.arange(9), DIST_SEED)
    assert same_bits(keys.cpu().numpy(), np.take_along_axis(K, order, axis=1))
    first = sample_items(dev(P), dev(Q), None, users, 1, seed=DIST_SEED, draw_ids=did)[0]
    assert torch.equal(first[:, 0], items[:, 0])


# ---- 7. T -> 0 is recommend -------------------------------------------------------------------------------------------
def test_cold_limit_is_recommend():
    """T = 2^-20 on a table whose scores are distinct multiples of 0.01 (every gap exceeds 1e-3, so 2^20 times a gap
    is > 1000 against a noise within [-3, 17]): the model confirms on the CPU that the draw is the arg-max, and the
    device gives `recommend`'s items."""
    from revisit_bpr.recommend import recommend
    from revisit_bpr.sample import sample_items

    rng = np.random.default_rng(11)
    Q = np.zeros((I, 8), F)
    Q[:, 0], Q[:, 1] = rng.permutation(I) * F(0.01), rng.permutation(I) * F(0.01)
    P = np.zeros((U, 8), F)
    P[np.arange(U), np.arange(U) % 2] = 1 + (np.arange(U) % 3)
    c = case(32, False, 1.0)
    users = np.arange(U).astype(np.int32)
    S = chain_scores(P, Q)
    ok = sm.eligible(I, users, c.indptr, c.indices)
    top = np.sort(np.where(ok, S, -np.inf).astype(np.float64), axis=1)[:, ::-1][:, :11]
    with np.errstate(invalid="ignore"):
        gaps = -np.diff(top, axis=1)  # (a short row: inf or nan past its end)
    assert gaps[np.isfinite(gaps)].min() > 1e-3
    T = 2.0 ** -20
    model = sm.sample_rows(P, Q, None, users, 10, c.indptr, c.indices, T, SEED)[0]
    argmax = np.argsort(-np.where(ok, S, -np.inf).astype(np.float64), axis=1, kind="stable")[:, :10]
    argmax = np.where(np.take_along_axis(ok, argmax, axis=1), argmax, -1)
    assert np.array_equal(model, argmax)  # on the CPU first
    want = recommend(dev(P), dev(Q), None, dev(users), 10, *c.csr)
    got = sample_items(dev(P), dev(Q), None, dev(users), 10, *c.csr, temperature=T, seed=SEED)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert np.array_equal(got[0].cpu().numpy(), model)


# ---- 8. arguments and the model's door --------------------------------------------------------------------------------
def test_arguments_are_refused_with_nothing_launched():
    from revisit_bpr import native
    from revisit_bpr.sample import sample_items

    c = case(32, False, 1.0)
    users = dev(c.users)
    for kw in (dict(k=0), dict(k=129), dict(k=3, temperature=0.0), dict(k=3, temperature=-1.0),
               dict(k=3, temperature=float("inf")), dict(k=3, temperature=float("nan")),
               dict(k=3, draw_ids=torch.zeros(N_ROWS - 1, dtype=torch.int64, device="cuda")),
               dict(k=3, draw_ids=torch.zeros(N_ROWS, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            sample_items(*c.t, users, **kw)
    with pytest.raises(ValueError):
        sample_items(c.t[0].double(), c.t[1], None, users, 3)
    with pytest.raises(ValueError):
        sample_items(c.t[0], c.t[1], None, users.float(), 3)
    with pytest.raises(ValueError):
        sample_items(c.t[0], c.t[1], None, users, 3, c.csr[0].int(), c.csr[1])
    # the C entry point itself, with real device pointers: BPR_ERR_INVALID
    lib = native.load()
    out_i = torch.empty((N_ROWS, 3), dtype=torch.int32, device="cuda")
    out_s = torch.empty((N_ROWS, 3), dtype=torch.float32, device="cuda")
    for k, T in ((0, 1.0), (129, 1.0), (3, 0.0), (3, -1.0), (3, float("inf")), (3, float("nan"))):
        rc = lib.bpr_sample_rows(c.t[0].data_ptr(), c.t[1].data_ptr(), None, I, 32, users.data_ptr(), N_ROWS, None,
                                 None, None, k, T, 0, 1, None, 0, out_i.data_ptr(), out_s.data_ptr(), None, None,
                                 None)
        assert rc == -1


def test_engine_and_model_sample_items():
    from revisit_bpr.engine import Engine
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN
    from revisit_bpr.sample import sample_items

    c = case(32, True, 1.0)
    e = Engine(c.t[0].clone(), c.t[1].clone(), item_bias=c.t[2].clone())
    e.bind_seen_csr(*c.csr)
    users = dev(c.users)
    got = e.sample_items(users, 10, seed=SEED, return_keys=True)
    want = sample_items(*c.t, users, 10, *c.csr, seed=SEED, return_keys=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    raw = e.sample_items(users, 10, exclude_seen=False, seed=SEED)
    assert (raw[0][c.users == 2] > 0).all()  # the user who has seen everything still gets draws
    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        model.sample_items(torch.zeros(1, dtype=torch.int32, device="cuda"), 3)

