"""Fold-in with scored negatives (`bpr_fold_in_rows_scored`, revisit_bpr/foldin.py: sampler="dynamic" | "warp") on a
machine without a GPU: the numpy restatement of the definition (tests/foldin_scored_model.py) on hand-checked triples,
the control-flow model of the kernel against the definition, the launch plan (revisit-bpr_amd/csrc/
bpr_foldin_scored_plan.h through the test hook `bpr_test_foldin_scored_plan`, and alone under the host sanitizers), the
refusals of the entry point before a device is touched, and the Python wrapper's."""
import ctypes
import math
import pathlib
import subprocess

import numpy as np
import pytest

import dynamic_model as dm
import foldin_scored_model as fm
import warp_model as wm

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
FIELDS = ("G", "E", "block", "groups_per_block", "pf", "groups", "grid", "resident", "bitmap", "bm_words", "lds_bytes",
          "lds_max")
INVALID, UNSUPPORTED = -1, -3
AUTO, CSR, BITMAP = 0, 1, 2
GIVEN, UNIFORM, ADAPTIVE, DYNAMIC, WARP = 0, 1, 2, 3, 4
LDS_CU = 163_840


def lib():
    from revisit_bpr import native

    return native.load()


def plan(n, I, d, kind=WARP, cus=256, seen_mode=AUTO):
    fn = lib().bpr_test_foldin_scored_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 6)(n, I, d, cus, seen_mode, kind), out) == 0
    return dict(zip(FIELDS, out))


def adaptive_plan(n, I, d, cus=256, seen_mode=AUTO):
    fn = lib().bpr_test_foldin_adaptive_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 5)(n, I, d, cus, seen_mode), out) == 0
    return dict(zip(FIELDS, out))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------
def test_restatement_is_its_parts_triple_by_triple():
    """One row, walked by hand beside `restate`: the draw of every triple is the stand-alone model's on the row as it
    stands, the dynamic step is foldin_model.step (+ bias), the WARP step is L in the place of sigma(-x), a skipped
    triple leaves the row alone."""
    pr = fm.problem(50, 8, 3)
    Q, b, I = pr["Q"], pr["b"], 50
    r = 5  # 17 positives
    lo, hi = int(pr["indptr"][r]), int(pr["indptr"][r + 1])
    one = np.array([0, hi - lo], np.int64)
    items, seen = pr["items"][lo:hi], set(pr["items"][lo:hi].tolist())
    P0 = pr["P0"][r:r + 1]  # one of the rows scaled up: the positive's rank decides
    for kind, K in (("dynamic", 4), ("warp", 3)):
        for bias in (None, b):
            P, neg, tries, _ = fm.restate(kind, Q, bias, one, items, P0, 2, 0.05, 0.02, K, 1.0, 7, 1000)
            p = P0[0].astype(np.float64)
            bb = np.zeros(I) if bias is None else bias.astype(np.float64)
            stepped = skipped = 0
            for t in range(2 * (hi - lo)):
                i = int(items[t % (hi - lo)])
                if kind == "dynamic":
                    j = dm.pick(7, 1000 + t, 0, K, p[None], Q, bias, None, None, seen=seen)["item"]
                    assert neg[t] == j >= 1 and tries[t] == 0 and j not in seen
                    x = float(p @ (Q[i].astype(np.float64) - Q[j])) + bb[i] - bb[j]
                    p = p - 0.05 * (-(1.0 / (1.0 + math.exp(x))) * (Q[i].astype(np.float64) - Q[j]) + 0.02 * p)
                else:
                    dr = wm.draw(7, 1000 + t, 0, i, K, 1.0, p[None], Q, bias, None, None, seen=seen)
                    assert (neg[t], tries[t]) == (dr["item"], dr["tries"])
                    if dr["item"] < 0:
                        skipped += 1
                        assert tries[t] == 0
                        continue
                    stepped += 1
                    L = wm.weight((I - 1) - (hi - lo), dr["tries"])
                    assert L == dr["weight"]
                    p = p - 0.05 * (-L * (Q[i].astype(np.float64) - Q[dr["item"]]) + 0.02 * p)
            assert np.allclose(P[0], p, rtol=1e-12, atol=1e-14)
            if kind == "warp":
                assert stepped > 0 and skipped > 0  # (a skipped triple took no L2 step either: p would differ)


def test_restatement_edges_one_unseen_item_all_seen_and_candidates_one():
    pr = fm.problem(50, 8, 1)
    for kind in ("dynamic", "warp"):
        P, neg, tries, _ = fm.restate(kind, pr["Q"], None, pr["indptr"], pr["items"], pr["P0"], 1, 0.05, 0.0, 4, 1.0, 5, 0)
        lo, hi = int(pr["indptr"][-3]), int(pr["indptr"][-2])
        only = np.setdiff1d(np.arange(1, 50), pr["rows"][-2])
        assert len(only) == 1 and set(neg[lo:hi].tolist()) <= {int(only[0]), -1}
        if kind == "dynamic":
            assert (neg[lo:hi] == only[0]).all() and (neg[hi:] == 0).all() and (tries == 0).all()
        else:  # n_unseen = 1: every stepped triple has L = log 1 = 0 and reg = 0, so the row stands still
            assert (tries[lo:hi][neg[lo:hi] > 0] == 1).all() and np.array_equal(P[-2], pr["P0"][-2].astype(np.float64))
            assert (neg[hi:] <= 0).all()  # nothing unseen: item 0 (reported, never applied) or no violator
        assert np.array_equal(P[-1], pr["P0"][-1].astype(np.float64)) and np.array_equal(P[0], pr["P0"][0].astype(np.float64))
    # candidates = 1 under dynamic is the uniform draw: a_1, whatever the scores
    _, neg, _, _ = fm.restate("dynamic", pr["Q"], None, pr["indptr"], pr["items"], pr["P0"], 1, 0.05, 0.0, 1, 1.0, 5, 0)
    for r in range(1, pr["n"] - 1):
        seen = set(pr["rows"][r].tolist())
        for k in range(int(pr["indptr"][r]), int(pr["indptr"][r + 1])):
            a = dm.accepted(5, k, seen, 50, 1)
            assert neg[k] == (a[0] if a else dm.rank_pick(5, k, seen, 50))


@pytest.mark.parametrize("I, d, N", sorted(fm.RUN_SEED))
def test_free_running_cases_leave_no_triple_undecided(I, d, N):
    """What tests/test_gpu_foldin_scored.py's free-running comparison rests on: under either kind the model decides
    every triple of the committed cases, early violators, late violators and skips all occur under WARP, and the
    dynamic picks are not all a_1."""
    for kind in ("dynamic", "warp"):
        pr, (P, neg, tries, und) = fm.run_model(kind, I, d, N)
        assert not und.any(), (kind, int(und.sum()))
        assert not np.array_equal(P[1:-1], pr["P0"][1:-1].astype(np.float64))
        if kind == "warp":
            assert (tries == 1).any() and (tries > 1).any() and (neg == -1).any()
            assert ((neg == -1) == (tries == 0)).all()
        else:
            assert (neg[:int(pr["indptr"][-2])] >= 1).all() and (tries == 0).all()


# ---- 2. the control flow ---------------------------------------------------------------------------------------------
I_FLOW, EPOCHS = 50, 3
LENGTHS = [0, 1, 2, 3, 9, 17, 40, 48, 49]  # 48: one item unseen; 49: none, every draw is 0


def inputs(warp, seed=7, d=8, base=0):
    rng = np.random.default_rng(seed)
    hist = [np.sort(rng.choice(np.arange(1, I_FLOW), size=k, replace=False)) for k in LENGTHS]
    indptr = base + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    items = np.concatenate([np.zeros(base, np.int64)] + hist).astype(np.int32)
    Q = rng.normal(0, 0.5, (I_FLOW, d))
    Q[0] = 0
    unseen = [np.setdiff1d(np.arange(1, I_FLOW), h) for h in hist]

    def sampler(t, p, r):  # a pure function of (the counter, the LIVE row, the row's unseen items)
        if len(unseen[r]) == 0:
            return 0, (0.0 if warp else None)
        h = (t * 2654435761 + int(np.abs(p).sum() * 1e6)) % 1000003
        if warp and h % 5 == 0:
            return -1, 0.0  # no violator: the triple is skipped
        return int(unseen[r][h % len(unseen[r])]), (math.log(1 + h % 7) if warp else None)

    return Q, indptr, items, rng.normal(0, 0.1, (len(LENGTHS), d)), sampler


@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_asks_the_sampler_what_the_definition_asks(pf, groups, warp):
    Q, indptr, items, P0, sampler = inputs(warp)
    want, want_log = fm.flow(Q, indptr, items, P0, EPOCHS, 0.05, 0.05, sampler)
    n = len(LENGTHS)
    assert not np.array_equal(want[1:8], P0[1:8]) and np.array_equal(want[[0, 8]], P0[[0, 8]])  # the all-seen row stays
    if warp:  # skipped triples are asked about too, and change nothing
        asked = [sampler(t, p, r) for t, r, p in want_log]
        assert any(j == -1 for j, _ in asked) and any(L == 0.0 and j > 0 for j, L in asked)
    key = lambda rec: rec[0]  # noqa: E731
    for order in (None, list(range(n))[::-1], list(np.random.default_rng(pf).permutation(n))):
        got, log, dummies, steps = fm.pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.05, sampler, pf, groups, order,
                                               ring_rows=not warp)
        assert np.array_equal(got, want), (pf, groups, order)
        # every triple asked once, with the state the definition has just before it; per row in triple order
        assert len(log) == len(want_log) == EPOCHS * sum(LENGTHS)
        for (t, r, p), (t2, r2, p2) in zip(sorted(log, key=key), sorted(want_log, key=key)):
            assert (t, r) == (t2, r2) and np.array_equal(p, p2), t
        for r in range(n):
            assert [t for t, rr, _ in log if rr == r] == [t for t, rr, _ in want_log if rr == r]
        # a row costs its triples + pf steps of fill, + at most pf - 1 idle steps to ring slot 0
        rows_with_triples = sum(1 for k in LENGTHS if k)
        assert steps <= EPOCHS * sum(LENGTHS) + rows_with_triples * (2 * pf - 1)
        assert dummies <= (groups - 1) * steps
        if groups == 1:
            assert dummies == 0  # alone in its wave a group never draws for nothing


@pytest.mark.parametrize("warp", [False, True])
def test_pipeline_on_a_slice_of_a_larger_csr_and_with_bad_ids(warp):
    Q, indptr, items, P0, sampler = inputs(warp, base=5)
    kw = dict(ring_rows=not warp)
    want, _ = fm.flow(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler)
    got, _, _, _ = fm.pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler, 2, 2, **kw)
    assert np.array_equal(got, want)
    n = len(LENGTHS)
    order = [8, 99, 7, 6, 5, -1, 4, 3, 2, 1, 0][:n]  # entries out of range are passed over: rows 1 and 0 never come up
    got, log, _, _ = fm.pipeline(Q, indptr, items, P0, EPOCHS, 0.05, 0.0, sampler, 2, 2, order, **kw)
    kept = [r for r in order if 0 <= r < n]
    assert np.array_equal(got[kept], want[kept])
    untouched = [r for r in range(n) if r not in kept]
    assert untouched and np.array_equal(got[untouched], P0[untouched])
    assert {r for _, r, _ in log} <= set(kept)
    bad = items.copy()
    bad[int(indptr[4]) + 2] = I_FLOW + 3  # a positive out of range: its triple is drawn for but not applied
    want, want_log = fm.flow(Q, indptr, bad, P0, EPOCHS, 0.05, 0.0, sampler)
    got, log, _, _ = fm.pipeline(Q, indptr, bad, P0, EPOCHS, 0.05, 0.0, sampler, 4, 3, **kw)
    assert np.array_equal(got, want) and len(log) == len(want_log)


# ---- 3. the plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [DYNAMIC, WARP])
@pytest.mark.parametrize("d", [1, 32, 128, 129, 256, 1024])
def test_plan_is_the_adaptive_plan_but_for_depth_and_residency(d, kind):
    want_ge = {1: (32, 1), 32: (32, 1), 128: (32, 4), 129: (64, 4), 256: (64, 4), 1024: (64, 16)}[d]
    for I in (50, 65_536, 65_537, 131_072, 131_073):
        for mode in (AUTO, CSR, BITMAP):
            for n in (0, 1, 10 ** 6):
                p, a = plan(n, I, d, kind, seen_mode=mode), adaptive_plan(n, I, d, seen_mode=mode)
                assert (p["G"], p["E"]) == want_ge and p["block"] == 256 and p["groups_per_block"] == 256 // p["G"]
                assert p["pf"] == (2 if p["E"] <= 4 else 1)
                for f in ("bitmap", "bm_words", "lds_bytes", "lds_max"):
                    assert p[f] == a[f], f
                fits = I <= (65_536 if p["G"] == 32 else 131_072)
                assert p["bitmap"] == int(fits and mode != CSR)
                low = p["bitmap"] and (p["E"] == 16 or (p["E"] == 4 and kind == DYNAMIC))
                assert p["resident"] == min(3 if low else 4, LDS_CU // p["lds_bytes"] if p["bitmap"] else 4)
                assert p["resident"] * p["lds_bytes"] <= LDS_CU and p["lds_bytes"] <= p["lds_max"]
                cap = 256 * p["resident"] * p["groups_per_block"]
                assert p["groups"] == min(n, cap) and p["grid"] == -(-p["groups"] // p["groups_per_block"])
                assert n < 10 ** 6 or p["groups"] == cap  # beyond the grid cap
                assert (n, p["groups"], p["grid"]) != (0, 0, 1)


def test_plan_hook_refuses_bad_shapes():
    fn = lib().bpr_test_foldin_scored_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 6)(4, 50, 0, 0, 0, WARP), out) == INVALID
    assert fn((ctypes.c_int64 * 6)(4, 50, 1025, 0, 0, WARP), out) == UNSUPPORTED
    assert fn((ctypes.c_int64 * 6)(4, 0, 8, 0, 0, WARP), out) == INVALID
    assert fn((ctypes.c_int64 * 6)(4, 50, 8, 0, 3, WARP), out) == INVALID
    assert fn((ctypes.c_int64 * 6)(4, 50, 8, 0, 0, UNIFORM), out) == UNSUPPORTED


def test_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """bpr_foldin_scored_plan.h is plain C++: built into a program of its own with -fsanitize=address,undefined,
    tests/foldin_scored_plan_check.cpp runs clean."""
    exe = tmp_path / "foldin_scored_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "foldin_scored_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4. refusals without a device ------------------------------------------------------------------------------------
def rows(Q=1, bias=None, I=100, d=8, indptr=1, items=1, n=4, row_order=None, epochs=3, lr=0.05, alpha=0.0, kind=WARP,
         candidates=10, margin=1.0, P=1):
    """bpr_fold_in_rows_scored with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be
    refused before the device is touched, or n = 0, go through here."""
    return lib().bpr_fold_in_rows_scored(Q, bias, I, d, indptr, items, n, row_order, epochs, lr, alpha, kind, candidates,
                                         margin, None, None, 0, 0, P, None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw, status, word", [
    (dict(candidates=0), INVALID, b"candidates"), (dict(candidates=33), INVALID, b"candidates"),
    (dict(candidates=-1), INVALID, b"candidates"), (dict(kind=DYNAMIC, candidates=0), INVALID, b"candidates"),
    (dict(kind=DYNAMIC, candidates=33), INVALID, b"candidates"),
    (dict(margin=0.0), INVALID, b"margin"), (dict(margin=-1.0), INVALID, b"margin"), (dict(margin=NAN), INVALID, b"margin"),
    (dict(margin=INF), INVALID, b"margin"),
    (dict(kind=GIVEN), UNSUPPORTED, b"bpr_fold_in_rows'"), (dict(kind=UNIFORM), UNSUPPORTED, b"bpr_fold_in_rows'"),
    (dict(kind=ADAPTIVE), UNSUPPORTED, b"bpr_fold_in_rows_adaptive"), (dict(kind=5), UNSUPPORTED, b"kind 5"),
    (dict(kind=-1), UNSUPPORTED, b"kind -1"),
    (dict(Q=None), INVALID, b"NULL"), (dict(indptr=None), INVALID, b"NULL"), (dict(items=None), INVALID, b"NULL"),
    (dict(P=None), INVALID, b"NULL"), (dict(epochs=0), INVALID, b"epochs"), (dict(d=0), INVALID, b"d must be"),
    (dict(d=1025), UNSUPPORTED, b"1024"), (dict(n=-1), INVALID, b"n must be"), (dict(n=2 ** 31), INVALID, b"2^31"),
    (dict(I=0), INVALID, b"I must be"), (dict(I=2 ** 21, d=1024), UNSUPPORTED, b"I * d"),
    (dict(lr=NAN), INVALID, b"NaN"), (dict(alpha=NAN), INVALID, b"NaN"),
])
def test_bad_arguments_are_refused_without_a_device(kw, status, word):
    assert rows(**kw) == status
    err = lib().bpr_last_error()
    assert word in err and err.startswith(b"bpr_fold_in_rows_scored"), err


def test_margin_is_ignored_for_dynamic_and_no_rows_is_ok_but_still_validated():
    none = dict(Q=None, indptr=None, items=None, P=None, n=0)
    assert rows(**none) == 0 and rows(**none, kind=DYNAMIC, candidates=4) == 0
    for m in (0.0, -1.0, NAN, INF):
        assert rows(**none, kind=DYNAMIC, candidates=4, margin=m) == 0
        assert rows(**none, margin=m) == INVALID
    assert rows(**none, epochs=0) == INVALID
    assert rows(**none, d=1025) == UNSUPPORTED
    assert rows(**none, candidates=33) == INVALID
    assert rows(**none, kind=UNIFORM) == UNSUPPORTED
    for c in (1, 32):
        assert rows(**none, candidates=c) == 0 and rows(**none, kind=DYNAMIC, candidates=c) == 0


def test_the_test_hook_checks_seen_mode_and_the_other_entries_still_refuse_both_kinds():
    from revisit_bpr import native

    fn = lib().bpr_test_fold_in_rows_scored
    fn.restype = ctypes.c_int
    fn.argtypes = native.SIGNATURES["bpr_fold_in_rows_scored"][1] + [ctypes.c_int32, ctypes.c_void_p]
    args = (1, None, 100, 8, 1, 1, 4, None, 3, 0.05, 0.0, WARP, 10, 1.0, None, None, 0, 0, 1, None)
    assert fn(*args, 3, None) == INVALID and b"seen_mode" in lib().bpr_last_error()
    assert fn(*args, -1, None) == INVALID
    for kind, word in ((DYNAMIC, b"dynamic"), (WARP, b"WARP")):
        rc = lib().bpr_fold_in_rows(1, None, 100, 8, 1, 1, 4, None, 3, 0.05, 0.0, kind, None, None, 0, 0, 1, None)
        assert rc == UNSUPPORTED and word.lower() in lib().bpr_last_error().lower()


# ---- 5. the wrapper --------------------------------------------------------------------------------------------------
def small():
    torch = pytest.importorskip("torch")
    Q = torch.randn(6, 8, generator=torch.Generator().manual_seed(0))
    return torch, Q, torch.tensor([0, 2, 3], dtype=torch.int64), torch.tensor([1, 4, 2], dtype=torch.int32)


@pytest.mark.parametrize("sampler", ["dynamic", "warp"])
def test_wrapper_accepts_the_sampler_and_refuses_cpu_tensors(sampler):
    from revisit_bpr.foldin import fold_in

    torch, Q, indptr, items = small()
    with pytest.raises(RuntimeError, match="ROCm"):  # (on the parent commit: ValueError, "sampler must be ...")
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler=sampler)
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler=sampler, return_neg=True, return_draws=True,
                candidates=32, max_sampled=32, margin=0.5, _states=True, _seen_mode=1)


def test_wrapper_refuses_bad_sampler_arguments_before_any_device():
    from revisit_bpr.foldin import fold_in, snapshot_of

    torch, Q, indptr, items = small()
    neg = torch.ones(6, dtype=torch.int32)
    for bad, word in ((dict(sampler="dynamic", neg=neg), "exclude each other"),
                      (dict(sampler="warp", neg=neg), "exclude each other"),
                      (dict(sampler="dynamic", candidates=0), "candidates"),
                      (dict(sampler="dynamic", candidates=33), "candidates"),
                      (dict(sampler="warp", max_sampled=0), "max_sampled"),
                      (dict(sampler="warp", max_sampled=33), "max_sampled"),
                      (dict(sampler="warp", margin=0.0), "margin"), (dict(sampler="warp", margin=-1.0), "margin"),
                      (dict(sampler="warp", margin=NAN), "margin"), (dict(sampler="warp", margin=INF), "margin"),
                      (dict(sampler="warp", snapshot=snapshot_of(Q)), "snapshot"),
                      (dict(sampler="dynamic", snapshot=snapshot_of(Q)), "snapshot"),
                      (dict(sampler="uniform", return_draws=True), "return_draws"),
                      (dict(sampler="uniform", _states=True), "_states"),
                      (dict(sampler="adaptive", _states=True), "_states"),
                      (dict(sampler="WARP"), "sampler must be"), (dict(sampler="popular"), "sampler must be")):
        with pytest.raises(ValueError, match=word):
            fold_in(Q, None, indptr, items, epochs=2, lr=0.05, **bad)
    # the parameters of the other kind are not looked at
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler="dynamic", max_sampled=99, margin=-1.0)
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05, sampler="warp", candidates=99)
    with pytest.raises(RuntimeError, match="ROCm"):  # every default stays uniform
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05)
