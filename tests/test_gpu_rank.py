"""The fused ranking kernel (`bpr_rank_rows`, revisit-bpr_amd/csrc/bpr_rank.hip) and what is built on it
(revisit_bpr.ranks.rank_items, Engine.rank_items, Model.rank_items, evaluation.evaluate_ranked) on the GPU.

The yardstick is tests/rank_model.py (brute force in numpy, pinned on the CPU by tests/test_rank_cpu.py).  Contract
under test: for every target, rank = eligible items other than it that come before it in `recommend`'s order,
not_below = those that score at least as high, score = `recommend`'s bits; an ineligible target gets -1 / -1 / -inf;
the outputs a pure function of the inputs (not of the row order, the grouping of targets into rows, the slicing).

Shapes: I = 300 is three item tiles, the last with 44 items; n = 70 rows is two row tiles, the second partial;
d = 33 takes the element-load path and a padded chunk, d = 256 eight chunks."""

import numpy as np
import pytest
import torch

from rank_model import rank_rows, user_metrics

pytestmark = pytest.mark.gpu

U, I, N = 12, 300, 70
EDGE = np.array([127, 128, 129, 255, 256, 299], np.int32)  # both sides of the tile boundaries, the last item


def tmax():
    from revisit_bpr.ranks import RANK_TMAX

    return RANK_TMAX


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(P, Q, b, users, tptr, titems, indptr=None, indices=None, item_slices=0):
    from revisit_bpr.ranks import rank_items

    out = rank_items(gpu(P), gpu(Q), gpu(b), gpu(users), gpu(tptr), gpu(titems), gpu(indptr), gpu(indices),
                     item_slices=item_slices)
    torch.cuda.synchronize()
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.float32]
    assert all(o.shape == (len(titems),) for o in out)
    return tuple(o.cpu().numpy() for o in out)


def same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.int32), want[2].view(np.int32)))


def seen_csr(rng):
    """user 0 has seen nothing, user 1 everything, user 2 exactly the items at the tile boundaries, user 3 those
    and more; the rest a random third."""
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


def target_rows(rng, indptr, indices):
    """70 rows: users 0 .. 3 for sure, repeats; 0, 1 and RANK_TMAX targets in a row; a seen target, id 0, an id out
    of range and a duplicate."""
    users = rng.integers(0, U, N).astype(np.int32)
    users[:6] = [0, 1, 2, 3, 2, 5]
    users[N - 1] = users[7]
    tg = [rng.integers(1, I, rng.integers(1, 7)).astype(np.int32) for _ in range(N)]
    tg[0] = np.zeros(0, np.int32)
    tg[1] = np.array([17], np.int32)  # (of the user who has seen everything)
    tg[2] = rng.choice(np.arange(1, I), tmax(), replace=False).astype(np.int32)
    tg[3] = np.array([126, 127, 130, 254, 298, 299], np.int32)
    seen5 = indices[indptr[5]:indptr[6]]
    free5 = np.setdiff1d(np.arange(1, I), seen5)
    tg[5] = np.array([seen5[0], 0, free5[0], free5[1], free5[0], I], np.int32)  # seen, id 0, a duplicate, out of range
    tg[66] = rng.choice(np.arange(1, I), tmax(), replace=False).astype(np.int32)  # (in the second, partial row tile)
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
    return users, tptr, np.concatenate(tg).astype(np.int32)


@pytest.fixture(scope="module")
def exact():
    """Tables from {-4 .. 4} / 4 and biases from multiples of 1 / 4: every score is a multiple of 1 / 16 below 2^9,
    exact in fp32 in any order, and ties are plentiful.  The model's answers are computed once per (d, bias, csr)."""
    rng = np.random.default_rng(2024)
    indptr, indices = seen_csr(rng)
    users, tptr, titems = target_rows(rng, indptr, indices)
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
            want = rank_rows(S.astype(np.float32), users, tptr, titems, *((indptr, indices) if csr else (None, None)))
            cache[key] = (P, Q, b, want)
        return cache[key]

    return dict(users=users, tptr=tptr, titems=titems, indptr=indptr, indices=indices, case=case)


# ---- 1. exact against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", [8, 33, 128, 256])
def test_exact_against_the_model(exact, d, bias):
    users, tptr, titems = exact["users"], exact["tptr"], exact["titems"]
    for csr in (True, False):
        P, Q, b, want = exact["case"](d, bias, csr)
        ptr, idx = (exact["indptr"], exact["indices"]) if csr else (None, None)
        if csr:  # the data does hold what it is meant to
            assert (want[0][tptr[1]:tptr[2]] == -1).all() and (want[0][tptr[2]:tptr[3]] >= 0).sum() > 100
            assert (want[1] > want[0]).sum() > 50  # ties
            five = want[0][tptr[5]:tptr[6]]
            assert five[0] == five[1] == five[5] == -1 and five[2] == five[4] >= 0
        for s in (0, 1, 3):
            got = run(P, Q, b, users, tptr, titems, ptr, idx, item_slices=s)
            bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
            assert same(got, want), (d, bias, csr, s, bad[:8], got[0][bad[:8]], want[0][bad[:8]], got[1][bad[:8]],
                                     want[1][bad[:8]])


# ---- 2. the score chain is recommend's ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(7)
    out = {}
    for d in (33, 128):
        P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
        out[d] = (P, Q, rng.standard_normal(I).astype(np.float32))
    out["csr"] = seen_csr(rng)
    return out


@pytest.mark.parametrize("d", [33, 128])
def test_ranks_of_recommended_items_are_their_positions(floats, d):
    """Random normal tables, no exactness trick: the k = 128 items `recommend` returns, as targets, have ranks
    0 .. 127 in order and bit-equal scores (128 > RANK_TMAX: the wrapper splits every row on the way)."""
    from revisit_bpr.recommend import recommend

    P, Q, b = floats[d]
    indptr, indices = floats["csr"]
    users = np.arange(U, dtype=np.int32)
    items, scores = recommend(gpu(P), gpu(Q), gpu(b), gpu(users), 128, gpu(indptr), gpu(indices))
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert (items[1] == -1).all() and (items[0] > 0).all()  # seen everything / nothing
    tptr = np.arange(0, 128 * U + 1, 128, dtype=np.int64)
    for s in (0, 1, 3):
        rank, not_below, score = run(P, Q, b, users, tptr, items.reshape(-1), indptr, indices, item_slices=s)
        rank, score = rank.reshape(U, 128), score.reshape(U, 128)
        live = items >= 0
        assert np.array_equal(rank[live], np.broadcast_to(np.arange(128), (U, 128))[live])
        assert (rank[~live] == -1).all() and np.isneginf(score[~live]).all()
        assert np.array_equal(score.view(np.int32), scores.view(np.int32))
        assert np.array_equal(not_below.reshape(U, 128)[live], rank[live])  # (no exact ties in this data)


# ---- 3. invariance ------------------------------------------------------------------------------------------------
def test_rows_may_be_permuted_repeated_and_split(floats):
    P, Q, b = floats[128]
    indptr, indices = floats["csr"]
    rng = np.random.default_rng(9)
    users = rng.integers(0, U, N).astype(np.int32)
    tg = [rng.integers(1, I, rng.integers(0, 9)).astype(np.int32) for _ in range(N)]
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
    ref = run(P, Q, b, users, tptr, np.concatenate(tg), indptr, indices, item_slices=1)
    assert (ref[0] >= 0).sum() > 100
    for s in (0, 3):
        assert same(run(P, Q, b, users, tptr, np.concatenate(tg), indptr, indices, item_slices=s), ref), s
    # rows in another order: the same numbers, moved with their targets
    perm = rng.permutation(N)
    ptr_p = np.concatenate([[0], np.cumsum([len(tg[r]) for r in perm])]).astype(np.int64)
    got = run(P, Q, b, users[perm], ptr_p, np.concatenate([tg[r] for r in perm]), indptr, indices)
    back = np.concatenate([np.arange(tptr[r], tptr[r + 1]) for r in perm])
    assert same(got, tuple(x[back] for x in ref))
    # every row cut in two rows of the same user (one of them may be empty), and one target per row
    for cut in ("halves", "singles"):
        us, lens = [], []
        for r in range(N):
            parts = [len(tg[r]) // 2, len(tg[r]) - len(tg[r]) // 2] if cut == "halves" else [1] * len(tg[r])
            us += [users[r]] * len(parts)
            lens += parts
        ptr_c = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        assert same(run(P, Q, b, np.array(us, np.int32), ptr_c, np.concatenate(tg), indptr, indices), ref), cut


# ---- 4. long rows -------------------------------------------------------------------------------------------------
def test_long_rows_are_split_by_the_wrapper_and_refused_by_the_entry_point(exact):
    from revisit_bpr import native

    P, Q, b, _ = exact["case"](33, True)
    indptr, indices = exact["indptr"], exact["indices"]
    rng = np.random.default_rng(4)
    T = 2 * tmax() + 3
    users = np.array([4, 6, 4], np.int32)
    tg = [rng.choice(np.arange(1, I), T, replace=False).astype(np.int32), np.array([5, -3, 6], np.int32),
          rng.choice(np.arange(1, I), tmax() + 1, replace=False).astype(np.int32)]
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
    titems = np.concatenate(tg)
    S = (P.astype(np.float64) @ Q.T.astype(np.float64) + b).astype(np.float32)
    want = rank_rows(S, users, tptr, titems, indptr, indices)
    for s in (0, 1, 3):
        assert same(run(P, Q, b, users, tptr, titems, indptr, indices, item_slices=s), want), s
    # the same rows straight to the entry point: refused with a message, nothing runs
    lib = native.load()
    t = [gpu(x) for x in (P, Q, users, tptr, titems)]
    out = [torch.zeros(len(titems), dtype=torch.int32, device="cuda") for _ in range(2)]
    sc = torch.zeros(len(titems), device="cuda")
    rc = lib.bpr_rank_rows(t[0].data_ptr(), t[1].data_ptr(), None, I, 33, t[2].data_ptr(), 3, t[3].data_ptr(),
                           t[4].data_ptr(), None, None, 1, None, 0, out[0].data_ptr(), out[1].data_ptr(),
                           sc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and str(T).encode() in lib.bpr_last_error() and b"RANK_TMAX" in lib.bpr_last_error()
    assert not out[0].any() and not sc.any()


# ---- 5. evaluate_ranked -------------------------------------------------------------------------------------------
def test_evaluate_ranked_on_the_exact_data(exact):
    from revisit_bpr.evaluation import evaluate_fused, evaluate_ranked

    P, Q, b, want = exact["case"](33, True)
    users, tptr, titems, indptr = exact["users"], exact["tptr"], exact["titems"], exact["indptr"]
    args = tuple(gpu(x) for x in (P, Q, b, users, tptr, titems, indptr, exact["indices"]))
    fused = evaluate_fused(*args, ks=(5, 100))
    got = evaluate_ranked(*args, ks=(5, 100))
    assert set(got) == set(fused) and len(got) == 6
    for name, v in fused.items():
        print(name, got[name], v, got[name] - v)
    for name, v in fused.items():
        assert abs(got[name] - v) <= 1e-6, (name, got[name], v)
    assert 0.0 < got["ndcg@100"] < 1.0
    # a cutoff past the top-K kernel's, MAP, MRR, per-user values: the numpy model
    with pytest.raises(ValueError):
        evaluate_fused(*args, ks=(200,))
    ks = (5, 100, 200, 1000)
    n_seen = (indptr[1:] - indptr[:-1])[users]
    model = user_metrics(*want, tptr, titems, I, n_seen, ks)
    got, per = evaluate_ranked(*args, ks=ks, extra=True, per_user=True)
    assert set(per) == set(got) == set(model) - {"auc"}
    for name in got:
        assert per[name].shape == (N,)
        mine = per[name].cpu().numpy()
        print(name, got[name], model[name].mean(), np.abs(mine - model[name]).max())
        assert np.abs(mine - model[name]).max() <= 1e-6, name
        assert abs(got[name] - float(mine.mean())) <= 1e-9 and abs(got[name] - model[name].mean()) <= 1e-6, name
    assert got["recall@200"] <= got["recall@1000"] < 1.0 and 0.0 < got["map@200"] < 1.0 and 0.0 < got["mrr"] < 1.0


def test_evaluate_ranked_auc_and_keys_on_tie_free_data(floats):
    from revisit_bpr.evaluation import evaluate_ranked, evaluate_topk
    from revisit_bpr.metrics.auc import RocAucManySlow

    P, Q, b = floats[128]
    rng = np.random.default_rng(21)
    rows = [np.flatnonzero(rng.random(I - 1) < 0.3).astype(np.int32) + 1 for _ in range(U)]
    rows[0] = np.zeros(0, np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    users = rng.integers(0, U, N).astype(np.int32)
    tg = [rng.choice(np.setdiff1d(np.arange(1, I), rows[u]), rng.integers(1, 9), replace=False).astype(np.int32)
          for u in users]
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
    args = tuple(gpu(x) for x in (P, Q, b, users, tptr, np.concatenate(tg), indptr, indices))
    # dense masked logits, as the eval loop builds them
    logits = args[0][args[3].long()] @ args[1].T + args[2]
    target = torch.zeros_like(logits)
    for e, u in enumerate(users):
        logits[e, torch.from_numpy(rows[u]).long().cuda()] = -1e13
        target[e, torch.from_numpy(tg[e]).long().cuda()] = 1.0
    logits[:, 0] = -1e13
    live = logits.cpu().numpy()
    for e in range(N):  # tie-free: no two eligible scores of a row are equal
        v = live[e][live[e] > -1e12]
        assert len(np.unique(v)) == len(v) > 100
    got, per = evaluate_ranked(*args, auc=True, per_user=True)
    want_auc = RocAucManySlow().compute(logits, target)
    print("auc", got["auc"], float(want_auc.mean()), float((per["auc"].float() - want_auc).abs().max()))
    assert float((per["auc"].float() - want_auc).abs().max()) <= 1e-6
    assert abs(got["auc"] - float(want_auc.double().mean())) <= 1e-6
    dense = evaluate_topk(*args, auc=True, block=32)
    assert set(dense) == set(got) and len(got) == 16
    for name, v in dense.items():
        print(name, got[name], v, got[name] - v)
    for name, v in dense.items():
        assert abs(got[name] - v) <= 1e-6, (name, got[name], v)
    assert 0.0 < got["auc"] < 1.0


# ---- 6. public layers ---------------------------------------------------------------------------------------------
def test_engine_rank_items_is_rank_items_on_its_tables(floats):
    from revisit_bpr.engine import Engine
    from revisit_bpr.ranks import rank_items

    P, Q, b = (gpu(x) for x in floats[128])
    tptr_seen, tidx_seen = (gpu(x) for x in floats["csr"])
    users = torch.arange(U, dtype=torch.int32, device="cuda")
    tptr = torch.arange(0, 3 * U + 1, 3, dtype=torch.int64, device="cuda")
    titems = torch.randint(1, I, (3 * U,), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    e = Engine(P, Q, b)
    none = e.rank_items(users, tptr, titems)  # no CSR bound: only item 0 is left out
    assert all(torch.equal(x, y) for x, y in zip(none, rank_items(P, Q, b, users, tptr, titems)))
    e.bind_seen_csr(tptr_seen, tidx_seen)
    got, want = e.rank_items(users, tptr, titems), rank_items(P, Q, b, users, tptr, titems, tptr_seen, tidx_seen)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert (got[0][3:6] == -1).all() and not torch.equal(got[0], none[0])  # user 1 has seen everything
    raw = e.rank_items(users, tptr, titems, exclude_seen=False)
    assert all(torch.equal(x, y) for x, y in zip(raw, none))
    e.close()


def test_model_rank_items_syncs_and_adds_the_user_bias():
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF, ItemKNN
    from revisit_bpr.ranks import rank_items

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"all": 0.001},
                logits_model=MF(torch.nn.Embedding(data.num_users, 32, padding_idx=0),
                                torch.nn.Embedding(data.num_items, 32, padding_idx=0), item_bias=True,
                                user_bias=True)).cuda()
    with torch.no_grad():
        model.logits_model._user_bias.copy_(torch.randn(data.num_users, device="cuda"))
    sptr, sidx = gpu(data.indptr), gpu(data.indices)
    model.bind_seen_csr(sptr, sidx)
    users = torch.arange(0, data.num_users, dtype=torch.int32, device="cuda")
    tptr = torch.arange(0, 2 * data.num_users + 1, 2, dtype=torch.int64, device="cuda")
    titems = torch.randint(1, data.num_items, (2 * data.num_users,), dtype=torch.int32, device="cuda",
                           generator=torch.Generator("cuda").manual_seed(2))
    got = model.rank_items(users, tptr, titems)
    sd = model.state_dict()
    want = rank_items(sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"],
                      sd["logits_model._item_bias"], users, tptr, titems, sptr, sidx)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2] + torch.repeat_interleave(sd["logits_model._user_bias"], 2))
    assert (got[0] >= 0).any() and (got[0] == -1).any()
    knn = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        knn.rank_items(users[:1], tptr[:2], titems[:2])
