"""Fold-in with adaptive negatives (`bpr_fold_in_rows_adaptive`, revisit_bpr/foldin.py) on a machine without a GPU:
the argument validation of the entry point, the launch plan (revisit-bpr_amd/csrc/bpr_foldin_adaptive_plan.h through
the test hook `bpr_test_foldin_adaptive_plan`), the Python wrapper's refusals, `snapshot_of` against a numpy
restatement, and the control-flow model of the kernel (tests/foldin_adaptive_model.py) against the definition."""
import ctypes

import numpy as np
import pytest

from foldin_adaptive_model import pipeline, randoms, restate

FIELDS = ("G", "E", "block", "groups_per_block", "pf", "groups", "grid", "resident", "bitmap", "bm_words", "lds_bytes",
          "lds_max")
INVALID, UNSUPPORTED = -1, -3
AUTO, CSR, BITMAP = 0, 1, 2
LDS_CU = 163_840


def lib():
    from revisit_bpr import native

    return native.load()


def plan(n, I, d, cus=256, seen_mode=AUTO):
    fn = lib().bpr_test_foldin_adaptive_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 5)(n, I, d, cus, seen_mode), out) == 0
    return dict(zip(FIELDS, out))


def uniform_plan(n, d, cus=256):
    fn = lib().bpr_test_foldin_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * 8)()
    assert fn((ctypes.c_int64 * 3)(n, d, cus), out) == 0
    return dict(zip(FIELDS[:8], out))


def rows(Q=1, bias=None, I=100, d=8, order=1, sigma=1, indptr=1, items=1, n=4, row_order=None, epochs=3, lr=0.05,
         alpha=0.0, p=0.2, P=1):
    """bpr_fold_in_rows_adaptive with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be
    refused before the device is touched, or n = 0, go through here."""
    return lib().bpr_fold_in_rows_adaptive(Q, bias, I, d, order, sigma, indptr, items, n, row_order, epochs, lr, alpha,
                                           p, None, None, None, 0, 0, P, None)


# ---- argument validation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, status, word", [
    (dict(order=None), INVALID, b"order"), (dict(sigma=None), INVALID, b"sigma"),
    (dict(p=0.0), INVALID, b"p not in"), (dict(p=1.0), INVALID, b"p not in"), (dict(p=-0.2), INVALID, b"p not in"),
    (dict(p=float("nan")), INVALID, b"p not in"), (dict(I=2 ** 30 + 2, d=1), UNSUPPORTED, b"2^30"),
    (dict(Q=None), INVALID, b"NULL"), (dict(indptr=None), INVALID, b"NULL"), (dict(items=None), INVALID, b"NULL"),
    (dict(P=None), INVALID, b"NULL"), (dict(epochs=0), INVALID, b"epochs"), (dict(d=0), INVALID, b"d must be"),
    (dict(d=1025), UNSUPPORTED, b"1024"), (dict(n=-1), INVALID, b"n must be"), (dict(n=2 ** 31), INVALID, b"2^31"),
    (dict(I=0), INVALID, b"I must be"), (dict(I=2 ** 21, d=1024), UNSUPPORTED, b"I * d"),
    (dict(lr=float("nan")), INVALID, b"NaN"),
])
def test_bad_arguments_are_refused_without_a_device(kw, status, word):
    assert rows(**kw) == status
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_the_largest_item_count_is_not_refused_for_its_size():
    assert rows(I=2 ** 30 + 1, d=1, n=0) == 0  # I - 1 == 2^30 passes the bound (n = 0: nothing else is touched)


def test_no_rows_is_ok_without_tables_but_still_validated():
    none = dict(Q=None, order=None, sigma=None, indptr=None, items=None, P=None, n=0)
    assert rows(**none) == 0
    assert rows(**none, epochs=0) == INVALID
    assert rows(**none, d=1025) == UNSUPPORTED
    assert rows(**none, p=1.5) == INVALID
    assert rows(**none, I=2 ** 30 + 2, d=1) == UNSUPPORTED


def test_the_uniform_entry_still_refuses_adaptive():
    rc = lib().bpr_fold_in_rows(1, None, 100, 8, 1, 1, 4, None, 3, 0.05, 0.0, 2, None, None, 0, 0, 1, None)
    assert rc == UNSUPPORTED and b"adaptive" in lib().bpr_last_error()


# ---- the plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_plan_group_shape_is_the_uniform_kernels(d):
    p, u = plan(1000, 2000, d), uniform_plan(1000, d)
    assert (p["G"], p["E"], p["block"], p["groups_per_block"]) == (u["G"], u["E"], u["block"], u["groups_per_block"])
    assert p["G"] * p["E"] >= d and p["pf"] >= 1


@pytest.mark.parametrize("d", [8, 128, 256])
@pytest.mark.parametrize("I", [50, 20_109, 131_072, 10 ** 6])
def test_plan_grid_never_exceeds_the_rows_and_is_capped_by_the_cus(d, I):
    gpb = plan(1, I, d)["groups_per_block"]
    for n in (0, 1, gpb - 1, gpb, gpb + 1, 1000, 10_000, 138_493, 2 ** 31 - 1):
        for cus in (1, 8, 256, 304):
            p = plan(n, I, d, cus)
            cap = cus * p["resident"] * gpb
            assert p["groups"] == min(n, cap)
            assert p["grid"] == -(-p["groups"] // gpb) <= cus * p["resident"]
            assert (p["grid"] - 1) * gpb < max(p["groups"], 1)  # no workgroup without a group


@pytest.mark.parametrize("d", [8, 256])
def test_plan_seen_structure_flips_exactly_where_the_bitmaps_stop_fitting(d):
    gpb, lds_max = plan(1, 50, d)["groups_per_block"], plan(1, 50, d)["lds_max"]

    def need(I):  # bytes of a workgroup's bitmaps: I bits per group in whole 16-byte vectors
        return -(-(-(-I // 32)) // 4) * 16 * gpb

    last = max(I for I in range(lds_max * 8 // gpb - 256, lds_max * 8 // gpb + 256) if need(I) <= lds_max)
    assert need(last) <= lds_max < need(last + 1)
    for I in (1, 2, 50, 300, 20_109, last - 1, last):
        p = plan(100, I, d)
        assert p["bitmap"] == 1 and p["lds_bytes"] == need(I) == p["bm_words"] * 4 * gpb, I
        assert p["bm_words"] % 4 == 0 and p["bm_words"] * 32 >= I
        assert plan(100, I, d, seen_mode=BITMAP) == p
        c = plan(100, I, d, seen_mode=CSR)
        assert (c["bitmap"], c["bm_words"], c["lds_bytes"]) == (0, 0, 0)
    for I in (last + 1, last + 2, 10 ** 6):
        for mode in (AUTO, BITMAP, CSR):  # a forced bitmap that does not fit is not taken
            p = plan(100, I, d, seen_mode=mode)
            assert (p["bitmap"], p["bm_words"], p["lds_bytes"]) == (0, 0, 0), (I, mode)


@pytest.mark.parametrize("d", [8, 128, 256, 1024])
def test_plan_lds_fits_the_cu_and_resident_is_consistent(d):
    for I in (2, 50, 300, 20_109, 41_140, 65_536, 65_537, 131_072, 131_073, 10 ** 6):
        for mode in (AUTO, CSR, BITMAP):
            p = plan(10 ** 6, I, d, seen_mode=mode)
            assert 0 <= p["lds_bytes"] <= p["lds_max"] <= LDS_CU
            assert 1 <= p["resident"] <= uniform_plan(1, d)["resident"]
            assert p["resident"] * p["lds_bytes"] <= LDS_CU
            if p["bitmap"]:  # as many workgroups as the uniform kernel's cap, or as the CU's LDS holds
                assert p["resident"] == min(uniform_plan(1, d)["resident"], LDS_CU // p["lds_bytes"])
            else:
                assert p["resident"] == uniform_plan(1, d)["resident"]


def test_plan_hook_refuses_bad_shapes():
    fn = lib().bpr_test_foldin_adaptive_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 5)(4, 50, 0, 0, 0), out) == INVALID
    assert fn((ctypes.c_int64 * 5)(4, 50, 1025, 0, 0), out) == UNSUPPORTED
    assert fn((ctypes.c_int64 * 5)(4, 0, 8, 0, 0), out) == INVALID
    assert fn((ctypes.c_int64 * 5)(4, 50, 8, 0, 3), out) == INVALID


# ---- the wrapper -----------------------------------------------------------------------------------------------------
def small():
    torch = pytest.importorskip("torch")
    Q = torch.randn(6, 8, generator=torch.Generator().manual_seed(0))
    return torch, Q, torch.tensor([0, 2, 3], dtype=torch.int64), torch.tensor([1, 4, 2], dtype=torch.int32)


def test_wrapper_refuses_cpu_tensors():
    from revisit_bpr.foldin import fold_in, snapshot_of

    torch, Q, indptr, items = small()
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler="adaptive")
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler="adaptive", snapshot=snapshot_of(Q),
                return_neg=True, return_draws=True)


def test_wrapper_refuses_bad_sampler_arguments():
    from revisit_bpr.foldin import fold_in, snapshot_of

    torch, Q, indptr, items = small()
    order, sigma = snapshot_of(Q)
    ok = dict(epochs=2, lr=0.05, sampler="adaptive")
    for bad in (dict(neg=torch.ones(6, dtype=torch.int32)), dict(sampler="popular"), dict(sampler="ADAPTIVE"),
                dict(adaptive_p=0.0), dict(adaptive_p=1.0), dict(adaptive_p=-0.1), dict(adaptive_p=float("nan")),
                dict(snapshot=(order.long(), sigma)), dict(snapshot=(order, sigma.double())),
                dict(snapshot=(order[:, :5], sigma)), dict(snapshot=(order[:7], sigma)),
                dict(snapshot=(order.t().contiguous(), sigma)), dict(snapshot=(order, sigma[:7])),
                dict(snapshot=(order.reshape(-1), sigma)),
                dict(sampler="uniform", return_draws=True), dict(sampler="uniform", snapshot=(order, sigma))):
        args = dict(ok)
        args.update(bad)
        with pytest.raises(ValueError):
            fold_in(Q, None, indptr, items, **args)


def test_snapshot_of_is_a_stable_descending_argsort_and_the_unbiased_std():
    from revisit_bpr.foldin import snapshot_of

    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    Q = rng.normal(0, 0.5, (40, 5)).astype(np.float32)
    Q[0] = 0
    Q[:, 1] = np.round(Q[:, 1])  # a column of ties: a handful of distinct values
    Q[:, 2] = 0.25               # and one of nothing else
    assert len(np.unique(Q[:, 1])) < 8
    order, sigma = snapshot_of(torch.from_numpy(Q))
    assert order.dtype == torch.int32 and tuple(order.shape) == (5, 40) and order.is_contiguous()
    assert sigma.dtype == torch.float32 and tuple(sigma.shape) == (5,)
    for f in range(5):  # descending by value, ties by ascending id, every row 0..I-1 (the pad row too)
        want = sorted(range(40), key=lambda i: (-float(Q[i, f]), i))
        assert order[f].tolist() == want, f
    assert order[2].tolist() == list(range(40))
    c = Q[1:].astype(np.float64) - Q[1].astype(np.float64)  # the engine's shifted sums (csrc/bpr_sort_shared.h)
    n = Q.shape[0] - 1
    want_sigma = np.sqrt(np.maximum((c * c).sum(axis=0) - c.sum(axis=0) ** 2 / n, 0.0) / (n - 1)).astype(np.float32)
    assert np.array_equal(sigma.numpy(), want_sigma)
    # which is the unbiased std over rows 1.. (float64 to fp32 rounding apart), and 0 for the constant column
    assert np.allclose(want_sigma, Q[1:].astype(np.float64).std(axis=0, ddof=1), rtol=2.0 ** -22, atol=0)
    assert sigma[2] == 0
    for bad in (torch.zeros(6), torch.zeros(6, 3, dtype=torch.float64), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            snapshot_of(bad)


# ---- the control-flow model ------------------------------------------------------------------------------------------
I, EPOCHS = 50, 3
LENGTHS = [0, 1, 2, 3, 9, 17, 40, 48, 49]  # 48: one item unseen; 49: none, every draw is 0


def inputs(seed=7, d=8, base=0):
    rng = np.random.default_rng(seed)
    hist = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)) for k in LENGTHS]
    indptr = base + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    items = np.concatenate([np.zeros(base, np.int64)] + hist).astype(np.int32)
    Q = rng.normal(0, 0.5, (I, d))
    Q[0] = 0
    unseen = [np.setdiff1d(np.arange(1, I), h) for h in hist]

    def sampler(t, p, rnd, r):  # a pure function of (counter's randoms, the LIVE row, the row's unseen items)
        assert rnd == randoms(t)  # the ring handed the consumer the randoms of ITS triple
        if len(unseen[r]) == 0:
            return 0
        return int(unseen[r][(rnd + int(np.abs(p).sum() * 1e6)) % len(unseen[r])])

    return Q, indptr, items, rng.normal(0, 0.1, (len(LENGTHS), d)), sampler


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_asks_the_sampler_what_the_definition_asks(pf, groups):
    Q, indptr, items, P0, sampler = inputs()
    want, want_log = restate(Q, indptr, items, P0, EPOCHS, 0.05, 0.05, sampler)
    n = len(LENGTHS)
    assert not np.array_equal(want[1:8], P0[1:8]) and np.array_equal(want[[0, 8]], P0[[0, 8]])
    key = lambda rec: rec[0]  # noqa: E731
    for order in (None, list(range(n))[::-1], list(np.random.default_rng(pf).permutation(n))):
        got, log, dummies, steps = pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.05, sampler, pf, groups, order)
        assert np.array_equal(got, want), (pf, groups, order)
        # every triple asked once, with the state the definition has just before it; per row in triple order
        assert len(log) == len(want_log) == EPOCHS * sum(LENGTHS)
        for (t, r, p), (t2, r2, p2) in zip(sorted(log, key=key), sorted(want_log, key=key)):
            assert (t, r) == (t2, r2) and np.array_equal(p, p2), t
        for r in range(n):
            mine = [t for t, rr, _ in log if rr == r]
            assert mine == [t for t, rr, _ in want_log if rr == r]
        # a row costs its triples + pf steps of fill, + at most pf - 1 idle steps to ring slot 0
        rows_with_triples = sum(1 for k in LENGTHS if k)
        assert steps <= EPOCHS * sum(LENGTHS) + rows_with_triples * (2 * pf - 1)
        assert dummies <= (groups - 1) * steps
        if groups == 1:
            assert dummies == 0  # alone in its wave a group never draws for nothing


def test_pipeline_on_a_slice_of_a_larger_csr_and_with_bad_ids():
    Q, indptr, items, P0, sampler = inputs(base=5)
    want, _ = restate(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler)
    got, _, _, _ = pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler, 2, 2)
    assert np.array_equal(got, want)
    n = len(LENGTHS)
    order = [8, 99, 7, 6, 5, -1, 4, 3, 2, 1, 0][:n]  # entries out of range are passed over: rows 1 and 0 never come up
    got, log, _, _ = pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler, 2, 2, order)
    kept = [r for r in order if 0 <= r < n]
    assert np.array_equal(got[kept], want[kept])
    untouched = [r for r in range(n) if r not in kept]
    assert untouched and np.array_equal(got[untouched], P0[untouched])
    assert {r for _, r, _ in log} <= set(kept)
    bad = items.copy()
    bad[int(indptr[4]) + 2] = I + 3  # a positive out of range: its triple is drawn for but not applied
    want, want_log = restate(Q, indptr, bad, P0, EPOCHS, 0.05, 0.0, sampler)
    got, log, _, _ = pipeline(Q, indptr, bad, P0, EPOCHS, 0.05, 0.0, sampler, 4, 3)
    assert np.array_equal(got, want) and len(log) == len(want_log)
