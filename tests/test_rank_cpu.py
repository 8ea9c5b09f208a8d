"""The fused ranking entry points on a machine without a GPU: the launch plan (revisit-bpr_amd/csrc/bpr_rank_plan.h,
through the library's test hook `bpr_test_rank_plan`), the argument validation of `bpr_rank_rows` (nothing touches
the device before the arguments are checked), the Python wrapper's refusals, and the numpy model of the contract
(tests/rank_model.py) against oracle/metrics_np.py and the torch metric classes on a dense example."""
import ctypes

import numpy as np
import pytest

from rank_model import rank_rows, user_metrics

TR, TI = 64, 128  # rows of a workgroup, items of a tile (bpr_rank_plan.h)
FIELDS = ("slices", "row_tiles", "item_tiles", "tile_rows", "tile_items", "tmax", "lds", "pre_lds", "ws_bytes")


def lib():
    from revisit_bpr import native

    return native.load()


def plan(n, I, d=128, item_slices=0, cus=256):
    fn = lib().bpr_test_rank_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 3
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    bounds = (ctypes.c_int64 * 65)()
    assert fn((ctypes.c_int64 * 5)(n, I, d, item_slices, cus), out, bounds) == 0
    p = dict(zip(FIELDS, out))
    p["bounds"] = list(bounds[:p["slices"] + 1])
    return p


def workspace(n, I=20109, d=128, item_slices=0):
    out = ctypes.c_int64(-1)
    assert lib().bpr_rank_workspace(n, I, d, item_slices, ctypes.byref(out)) == 0
    return out.value


def rows(P=1, Q=1, I=100, d=8, users=1, n=4, tptr=1, titems=1, item_slices=0, ws=None, ws_bytes=0, rank=1, nb=1, score=1):
    """bpr_rank_rows with fake non-NULL pointers (1): only calls that must be refused before the device is touched,
    or n = 0, go through here."""
    return lib().bpr_rank_rows(P, Q, None, I, d, users, n, tptr, titems, None, None, item_slices, ws, ws_bytes, rank,
                               nb, score, None)


# ---- the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [1, 2, 127, 128, 129, 300, 5000, 20109, 41140, 1_000_003])
def test_slices_cover_the_items_exactly_once(I):
    for item_slices in (0, 1, 2, 3, 7, 64):
        for n in (1, 70, 1000):
            p = plan(n, I, item_slices=item_slices)
            b = p["bounds"]
            assert b[0] == 0 and b[-1] == I and len(b) == p["slices"] + 1
            assert all(lo < hi for lo, hi in zip(b, b[1:])), b  # disjoint, in order, none empty
            assert all(x % TI == 0 for x in b[:-1])  # whole tiles


def test_lds_fits_a_cu_for_every_row_up_to_tmax():
    from revisit_bpr.ranks import RANK_TMAX

    for d in (1, 33, 128, 1024):
        p = plan(1000, 20109, d=d, item_slices=64)
        assert p["tmax"] == RANK_TMAX >= 100  # (the LDS is sized for RANK_TMAX targets in each of the 64 rows)
        assert 0 < p["pre_lds"] < p["lds"] <= 163_840
        assert (p["tile_rows"], p["tile_items"]) == (TR, TI)
        # staged operands + scalars + masks + per row and target: 8 (score, id) + 4 bin + 4 tied + 2 place
        assert p["lds"] >= (TR + TI) * 36 * 4 + TR * 16 + TR * (RANK_TMAX * 18 + 4)


@pytest.mark.parametrize("item_slices", [0, 1, 2, 7, 64])
def test_workspace_is_monotone_in_n(item_slices):
    ns = [0, 1, 2, 63, 64, 65, 255, 256, 1000, 4096, 8191, 8192, 10_000, 16_000, 16_320, 16_321, 16_384, 20_000,
          138_493, 571_355]
    got = [workspace(n, item_slices=item_slices) for n in ns]
    assert all(b >= 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), list(zip(ns, got))
    if item_slices == 1:
        assert got[-1] == 0
    for n in (1, 100, 5000, 16_000, 16_384, 138_493):  # the choice's answer covers every call's own need
        assert plan(n, 20109)["ws_bytes"] <= workspace(n)


def test_plan_slices_by_the_row_tiles():
    assert plan(256 * TR, 20109)["slices"] == 1  # 256 row tiles: one per CU
    assert plan(256 * TR - TR + 1, 20109)["slices"] == 1
    assert plan(138_493, 20109)["slices"] == 1
    assert plan(255 * TR, 20109)["slices"] == 2
    assert plan(1, 20109)["slices"] == 64  # capped at 64
    assert plan(70, 300)["slices"] == 3  # ... and at the item tiles
    assert plan(10_000, 20109, item_slices=7)["slices"] == 7
    assert plan(10_000, 200, item_slices=7)["slices"] == 2  # no empty slices
    assert plan(0, 20109)["row_tiles"] == 0
    out = ctypes.c_int32(-1)
    for n, I, given in ((1, 20109, 0), (10_000, 20109, 0), (138_493, 20109, 0), (10_000, 200, 7)):
        assert lib().bpr_rank_slices(n, I, 128, given, ctypes.byref(out)) == 0
        p = plan(n, I, item_slices=given)
        assert out.value == p["slices"]
        assert workspace(n, I=I, item_slices=out.value) == p["ws_bytes"]
        assert p["ws_bytes"] == (0 if p["slices"] == 1 else n * p["tmax"] * 12)


# ---- the entry point's refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(P=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(users=None), b"NULL"), (dict(tptr=None), b"NULL"),
    (dict(d=0), b"d must be"), (dict(d=1025), b"1024"), (dict(I=0), b"I in"), (dict(n=-1), b"n must be"),
    (dict(n=2 ** 31), b"2^31"), (dict(item_slices=-1), b"item_slices"), (dict(item_slices=65), b"item_slices"),
    (dict(item_slices=4, I=5000, ws=None, ws_bytes=0), b"workspace"),
    (dict(item_slices=4, I=5000, ws=1, ws_bytes=4 * 112 * 12 - 1), b"workspace"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_rows_is_ok_without_tables():
    assert rows(P=None, Q=None, users=None, tptr=None, titems=None, rank=None, nb=None, score=None, n=0) == 0
    assert rows(P=None, Q=None, users=None, tptr=None, n=0, d=0) == -1  # (still validated)
    out = ctypes.c_int64()
    assert lib().bpr_rank_workspace(4, 100, 8, 0, None) == -1
    assert lib().bpr_rank_workspace(4, 0, 8, 0, ctypes.byref(out)) == -1 and lib().bpr_last_error()


def test_wrapper_checks_its_arguments_on_any_device():
    torch = pytest.importorskip("torch")
    from revisit_bpr.ranks import rank_items

    ok = dict(P=torch.zeros(4, 8), Q=torch.zeros(6, 8), item_bias=None, users=torch.zeros(2, dtype=torch.int32),
              tgt_indptr=torch.tensor([0, 2, 3]), tgt_items=torch.tensor([1, 4, 2], dtype=torch.int32),
              seen_indptr=torch.zeros(5, dtype=torch.int64), seen_indices=torch.zeros(0, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ROCm"):  # well-formed, but there is no CPU path
        rank_items(**ok)
    for bad in (dict(P=ok["P"].double()), dict(Q=torch.zeros(6, 4)), dict(Q=torch.zeros(6)),
                dict(item_bias=torch.zeros(5)), dict(item_bias=torch.zeros(6, dtype=torch.float64)),
                dict(users=torch.zeros(2)), dict(tgt_indptr=torch.tensor([0, 2, 3], dtype=torch.int32)),
                dict(tgt_items=torch.tensor([1, 4, 2])), dict(tgt_indptr=torch.tensor([0, 3])),
                dict(seen_indptr=torch.zeros(4, dtype=torch.int64)),  # U + 1 = 5 entries are needed
                dict(seen_indptr=torch.zeros(5, dtype=torch.int32)), dict(seen_indices=torch.zeros(0, dtype=torch.int64)),
                dict(seen_indices=None)):
        with pytest.raises(ValueError):
            rank_items(**{**ok, **bad})


# ---- the model against the dense definitions ---------------------------------------------------------------------
def dense_case():
    rng = np.random.default_rng(11)
    U, I, d = 7, 40, 4
    S = (rng.standard_normal((U, d)) @ rng.standard_normal((I, d)).T).astype(np.float32)
    seen = [np.sort(rng.choice(np.arange(1, I), size=rng.integers(0, 12), replace=False)).astype(np.int32)
            for _ in range(U)]
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64)
    indices = np.concatenate(seen).astype(np.int32)
    users = np.array([3, 0, 6, 1, 5, 2], np.int32)
    tg = []
    for e, u in enumerate(users):
        unseen = np.setdiff1d(np.arange(1, I), seen[u])
        t = rng.choice(unseen, size=(0, 1, 3, 5, 2, 8)[e], replace=False)
        if e == 4 and len(seen[u]):
            t = np.append(t, seen[u][0])  # a held-out item the user has also seen: never retrieved
        tg.append(t.astype(np.int32))
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
    titems = np.concatenate(tg).astype(np.int32)
    logits = S[users].copy()
    target = np.zeros_like(logits)
    mask = np.ones_like(logits)
    for e, u in enumerate(users):
        logits[e, seen[u]] = -1e13
        mask[e, seen[u]] = 0
        target[e, tg[e]] = 1.0
    logits[:, 0] = -1e13
    mask[:, 0] = 0
    for e in range(len(users)):  # tie-free: the dense forms and the model break no tie differently
        live = logits[e][mask[e] != 0]
        assert len(np.unique(live)) == len(live)
    n_seen = (indptr[1:] - indptr[:-1])[users]
    return S, users, tptr, titems, indptr, indices, logits, target, mask, n_seen


def test_model_ranks_are_the_positions_in_the_sorted_row():
    S, users, tptr, titems, indptr, indices, logits, target, mask, _ = dense_case()
    rank, not_below, score = rank_rows(S, users, tptr, titems, indptr, indices)
    for e in range(len(users)):
        order = np.argsort(-logits[e], kind="stable")
        for p in range(tptr[e], tptr[e + 1]):
            if mask[e, titems[p]] == 0:
                assert rank[p] == not_below[p] == -1 and np.isneginf(score[p])
            else:
                assert order[rank[p]] == titems[p] and not_below[p] == rank[p] and score[p] == S[users[e], titems[p]]


def test_model_metrics_equal_the_oracle_and_the_metric_classes():
    torch = pytest.importorskip("torch")
    from oracle import metrics_np
    from revisit_bpr.metrics.auc import RocAucManySlow
    from revisit_bpr.metrics.ranking import MAP, NDCG, Precision, Recall

    S, users, tptr, titems, indptr, indices, logits, target, mask, n_seen = dense_case()
    I = S.shape[1]
    ks = (3, 10, 25)
    r = rank_rows(S, users, tptr, titems, indptr, indices)
    got = user_metrics(*r, tptr, titems, I, n_seen, ks)
    tl, tt, tm = torch.from_numpy(logits), torch.from_numpy(target), torch.from_numpy(mask)
    for k in ks:
        for name, np_fn, cls in (("ndcg", metrics_np.ndcg, NDCG), ("recall", metrics_np.recall, Recall),
                                 ("precision", metrics_np.precision, Precision)):
            assert np.allclose(got[f"{name}@{k}"], np_fn(logits, target, k), rtol=0, atol=1e-6), (name, k)
            assert np.allclose(got[f"{name}@{k}"], cls(k).compute(tl, tt).numpy(), rtol=0, atol=1e-6), (name, k)
        assert np.allclose(got[f"map@{k}"], MAP(k).compute(tl, tt).numpy(), rtol=0, atol=1e-6), k
    # AUC: masked entries as negatives (the eval loop's logits) ...
    want = metrics_np.roc_auc_many(logits, target)
    assert np.isnan(want[0]) and np.isnan(got["auc"][0])  # the user without positives: 0 / 0
    assert np.allclose(got["auc"][1:], want[1:], rtol=0, atol=1e-6)
    assert np.allclose(got["auc"][1:], RocAucManySlow().compute(tl, tt).numpy()[1:], rtol=0, atol=1e-6)
    # ... and over the eligible items only (the metric classes' mask argument)
    elig = user_metrics(*r, tptr, titems, I, n_seen, ks, masked_negatives=False)
    want = metrics_np.roc_auc_many(logits, target * mask, mask)
    assert np.allclose(elig["auc"][1:], want[1:], rtol=0, atol=1e-6)
    assert np.allclose(elig["auc"][1:], RocAucManySlow().compute(tl, tt * tm, tm).numpy()[1:], rtol=0, atol=1e-6)
    # MRR: the first relevant position of the dense ranking
    for e in range(1, len(users)):
        rel = metrics_np.prepare_target(logits[e:e + 1], (target * mask)[e:e + 1])[0]
        assert got["mrr"][e] == 1.0 / (1 + int(np.flatnonzero(rel)[0]))
    assert got["mrr"][0] == 0.0


def test_model_counts_ties_by_the_rule():
    """Equal scores: the lower id comes first; not_below also counts the equal ones that come after."""
    S = np.array([[9, 1, 2, 2, 2, 0, 2, 3]], np.float32)  # item 0 is never eligible
    users, tptr = np.array([0], np.int32), np.array([0, 4], np.int64)
    titems = np.array([4, 2, 7, 4], np.int32)
    indptr, indices = np.array([0, 1], np.int64), np.array([6], np.int32)  # item 6 (a 2) is seen
    rank, not_below, score = rank_rows(S, users, tptr, titems, indptr, indices)
    assert rank.tolist() == [3, 1, 0, 3] and not_below.tolist() == [3, 3, 0, 3] and score.tolist() == [2, 2, 3, 2]
