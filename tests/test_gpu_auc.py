"""The evaluation kernel (`bpr_auc_rows`, revisit-bpr_amd/csrc/bpr_eval.hip: k_auc_rows) and the `auc` built on it
(evaluation.evaluate_topk, evaluate_ranked) held to an exact all-pairs count on the GPU.

The yardstick is tests/auc_model.py (numpy, integer counts; pinned on the CPU by tests/test_auc_model_cpu.py); the rows
come from tests/auc_cases.py.  Every comparison with the model is BIT EQUALITY of the float32 result, and every row
keeps T (I - T) <= 2^24, where one miscounted pair changes those bits (test_auc_model_cpu.py::
test_one_pair_changes_the_float32_up_to_2_pow_24): `launch` asserts that condition on its inputs before it launches, so
an edit of the shapes cannot void the file unnoticed.  No id out of [0, I) is ever passed: that is a documented
precondition of the entry point, which cannot check it.

  1  counts at the kernel's constants: T in {1, 2, 255, 256, 257, 1023, 4095, 4096}, I - T in {1, 255, 256, 257}
     (4,096 too for the two largest T), I = 2, I = 200; score classes a (distinct), b (multiples of 1 / 2), c (all
     equal), d (b with -1e13 entries), e (b with +-inf, +-0, subnormals); target lists in random and in ascending order;
     rows permuted, and alone
  2  not computed: T = 0, T = I, T = 4097 are NaN and leave their neighbours alone
  3  NaN scores, twice with launches of another shape in between that overwrite all 32 KB of LDS
  4  evaluate_topk (GPU and CPU tensors, user by user and whole) and evaluate_ranked on one adversarial dataset"""
import numpy as np
import pytest
import torch

from auc_cases import (CLASSES, MIXED_I, TN_MAX, Rows, boundary_rows, boundary_shapes, family, mixed_rows, one_user,
                       scores_of, whole_call)
from auc_model import bits

pytestmark = pytest.mark.gpu


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def launch(scores, ptr, items):
    """bpr_auc_rows on [n, I] scores and a CSR of target ids -> float32 [n].  Refuses inputs on which bit equality
    would not see a single pair, and ids the entry point must not be given."""
    from revisit_bpr import native

    n, I = scores.shape
    T = np.diff(ptr)
    assert scores.dtype == np.float32 and ptr.dtype == np.int64 and items.dtype == np.int32 and len(ptr) == n + 1
    assert (np.minimum(T, 4097) * np.maximum(I - T, 0) <= TN_MAX).all(), "T (I - T) <= 2^24: one pair is one ulp"
    used = items[ptr[0]:ptr[-1]]
    assert used.size == 0 or (used.min() >= 0 and used.max() < I), "ids in [0, I)"
    ts, tp, ti = gpu(scores), gpu(ptr), gpu(items if items.size else np.zeros(1, np.int32))
    out = torch.full((n,), 7.0, device="cuda", dtype=torch.float32)
    native.check(native.load().bpr_auc_rows(ts.data_ptr(), n, I, tp.data_ptr(), ti.data_ptr(), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_bits(got, rows, what):
    bad = np.flatnonzero(bits(got) != bits(rows.value))
    assert bad.size == 0, (what, rows.I, [(int(rows.T[r]), int(rows.wins[r]), float(got[r]), float(rows.value[r]),
                                           float(got[r]) * float(rows.T[r] * rows.n_neg[r])) for r in bad[:6]])


# ---- 1. counts at the kernel's boundaries ----------------------------------------------------------------------------
def test_the_shapes_are_the_boundaries():
    shapes = boundary_shapes()
    assert {T for T, _ in shapes} == {1, 2, 7, 255, 256, 257, 1023, 4095, 4096}
    assert {I - T for T, I in shapes} == {1, 193, 255, 256, 257, 4096}
    assert max(T * (I - T) for T, I in shapes) == TN_MAX and (1, 2) in shapes and (7, 200) in shapes
    groups = boundary_rows("b")
    assert sum(g.n for g in groups) == len(shapes) == 35  # 8 x 4 (I = 2 is one of them), the two of 2^24, I = 200
    assert max(len(set(g.T.tolist())) for g in groups) >= 3  # rows of different T in one launch


@pytest.mark.parametrize("cls", CLASSES)
def test_counts_at_the_boundaries(cls):
    groups = boundary_rows(cls)
    flat = np.concatenate([g.scores.ravel() for g in groups])
    tiny = np.float32(2.0 ** -126)
    if cls == "a":
        assert all(len(np.unique(g.scores[r])) == g.I for g in groups for r in range(g.n))
    if cls == "c":
        assert all((g.wins == 0).all() and (g.value == 0).all() for g in groups)  # AUC is exactly 0
    if cls == "d":
        assert any(g.scores[r, g.items[g.ptr[r]]] == np.float32(-1e13) for g in groups for r in range(g.n))
    if cls == "e":
        assert np.isinf(flat).any() and (np.signbit(flat) & (flat == 0)).any() and ((np.abs(flat) < tiny) & (flat != 0)).any()
    if cls in "bde":  # ties across positives and negatives: '>' and '>=' count differently
        g = groups[-1]
        pos = g.scores[0][g.items[g.ptr[0]:g.ptr[1]]]
        assert np.intersect1d(pos, np.delete(g.scores[0], g.items[g.ptr[0]:g.ptr[1]])).size >= 5
        assert len(np.unique(pos)) < len(pos)
    assert not np.isnan(flat).any()
    for g in groups:
        got = launch(g.scores, g.ptr, g.items)
        assert_bits(got, g, cls)
        again = launch(g.scores, g.ptr, g.items_sorted)  # the tie-break by list index does not leak into the value
        assert np.array_equal(bits(again), bits(got)), (cls, g.I)


def test_signed_zeros_and_subnormals_by_hand():
    s = np.array([[0.0, -0.0, 2.0 ** -149, 0.0, -(2.0 ** -149), 1.0]], np.float32)
    rows = Rows(s, [np.array([0, 2], np.int32)])
    # +0 against -0 and 0: no win; the subnormal beats -0, 0 and its negative (a flushed compare would lose them)
    assert (rows.wins[0], rows.T[0], rows.n_neg[0]) == (4, 2, 4)
    assert_bits(launch(rows.scores, rows.ptr, rows.items), rows, "hand")


@pytest.mark.parametrize("cls", CLASSES)
def test_rows_are_independent(cls):
    rows = mixed_rows(cls)
    assert rows.n == 40 and rows.I == MIXED_I and {1, 2, 255, 256, 257, 1023, 4095, 4096} <= set(rows.T.tolist())
    got = launch(rows.scores, rows.ptr, rows.items)
    assert_bits(got, rows, cls)
    order = np.random.default_rng(1).permutation(rows.n)
    perm = rows.take(order)
    assert np.array_equal(bits(launch(perm.scores, perm.ptr, perm.items)), bits(got[order]))
    for r in (int(np.flatnonzero(rows.T == 4096)[0]), int(np.flatnonzero(rows.T == 257)[0]), rows.n - 1):
        alone = rows.take([r])
        assert bits(launch(alone.scores, alone.ptr, alone.items))[0] == bits(got)[r], (cls, r)
    # a CSR that does not start at 0: the rows 5 .. 12 of the same arrays
    sub = launch(rows.scores[5:12], rows.ptr[5:13], rows.items)
    assert np.array_equal(bits(sub), bits(got[5:12]))


# ---- 2. not computed -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I, Ts", [(1, [1, 0]), (5, [2, 0, 5, 1, 4]), (4096, [7, 4096, 0, 4095]),
                                   (4200, [1, 4097, 4096, 0, 4097, 300])])
def test_not_computed_is_nan_and_leaves_the_neighbours_alone(I, Ts):
    rng = np.random.default_rng(I)
    targets = [np.sort(rng.choice(I, T, replace=False)).astype(np.int32) for T in Ts]
    rows = Rows(np.stack([scores_of("b", rng, I) for _ in Ts]), targets)
    want_nan = np.array([T == 0 or T == I or T > 4096 for T in Ts])
    assert np.array_equal(np.isnan(rows.value), want_nan)
    got = launch(rows.scores, rows.ptr, rows.items)
    assert np.array_equal(np.isnan(got), want_nan), got
    assert_bits(got, rows, "not computed")


# ---- 3. NaN scores ---------------------------------------------------------------------------------------------------
def nan_case():
    """Class (b) rows of I = 1,000 with NaN among the negatives, the positives, both, everywhere; T = 40 (one
    positive per thread at most) and T = 300 (two for some threads)."""
    rng = np.random.default_rng(33)
    I, plans = 1000, []
    for T in (40, 300):
        for n_pos, n_neg in ((0, 1), (0, 60), (1, 0), (17, 0), (1, 1), (17, 60), (T, 0), (0, I - T)):
            plans.append((T, n_pos, n_neg))
    plans += [(1, 1, 0), (1, 1, 999), (40, 40, 960), (300, 300, 700)]  # the only positive; every score
    targets = [rng.choice(I, T, replace=False).astype(np.int32) for T, _, _ in plans]
    scores = np.stack([scores_of("b", rng, I) for _ in plans])
    for r, (T, n_pos, n_neg) in enumerate(plans):
        t = targets[r]
        scores[r, rng.choice(t, n_pos, replace=False)] = np.nan
        scores[r, rng.choice(np.setdiff1d(np.arange(I), t), n_neg, replace=False)] = np.nan
    rows = Rows(scores, targets)
    every = np.isnan(scores).all(1)
    assert every.sum() == 3 and (rows.value[every] == 0).all()  # T (I - T) is nonzero: 0.0, not NaN
    assert not np.isnan(rows.value).any() and (rows.wins > 0).sum() == len(plans) - 8
    return rows


def dirty_lds():
    """512 rows of another shape (I = 4,200, T = 4,096 distinct large scores): every workgroup writes all of its
    16 KB of sorted positives and 16 KB of bins."""
    from revisit_bpr import native

    n, I, T = 512, 4200, 4096
    scores = (torch.rand(n, I, device="cuda") + 1.0) * 1e30
    ptr = torch.arange(n + 1, device="cuda", dtype=torch.int64) * T
    items = torch.arange(T, device="cuda", dtype=torch.int32).repeat(n)
    out = torch.empty(n, device="cuda")
    native.check(native.load().bpr_auc_rows(scores.data_ptr(), n, I, ptr.data_ptr(), items.data_ptr(), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_nan_scores_win_nothing_and_the_answer_does_not_depend_on_what_lds_held():
    rows = nan_case()
    first = launch(rows.scores, rows.ptr, rows.items)
    dirty_lds()
    dirty_lds()
    second = launch(rows.scores, rows.ptr, rows.items)
    assert np.array_equal(bits(first), bits(second)), (first, second)
    assert_bits(first, rows, "nan")
    assert_bits(launch(rows.scores, rows.ptr, rows.items_sorted), rows, "nan, ascending ids")


# ---- 4. the evaluation family on one adversarial dataset -------------------------------------------------------------
def test_evaluate_topk_user_by_user_on_both_devices():
    f = family()
    wins, T, n_neg, value = f.model
    for e in range(f.E):
        on_gpu, on_cpu = one_user(f, e, "cuda"), one_user(f, e, "cpu")
        print(e, int(T[e]), int(wins[e]), float(on_gpu), float(on_cpu), float(value[e]))
        assert bits(on_gpu) == bits(value[e]), (e, float(on_gpu), float(value[e]), int(wins[e]), int(T[e]))
        assert bits(on_cpu) == bits(value[e]), (e, float(on_cpu), float(value[e]), int(wins[e]), int(T[e]))


def test_evaluate_topk_whole_call_in_blocks_of_seven():
    f = family()
    value = f.model[3]
    assert np.isnan(whole_call(f, (0, f.E), "cuda")) and np.isnan(whole_call(f, (0, f.E), "cpu"))  # a user without targets
    E = f.E - 1
    assert f.SORTED_FORM // 7 == (f.SORTED_FORM + 1) // 7 and E > 7  # the 4,097-target row shares a block with kernel rows
    want = float(np.mean(value[1:].astype(np.float64)))
    for device in ("cuda", "cpu"):
        got = whole_call(f, (1, f.E), device)
        print(device, got, want, abs(got - want), (E + 1) * 2.0 ** -24)
        # an fp32 running sum of E terms in [0, 1] and the final rounding
        assert abs(got - want) <= (E + 1) * 2.0 ** -24, (device, got, want)


def test_evaluate_ranked_auc_on_tied_data():
    from revisit_bpr.evaluation import evaluate_ranked

    f = family()
    wins, T, n_neg, _ = f.model
    assert np.isfinite(f.logits).all()
    _, per = evaluate_ranked(gpu(f.P), gpu(f.Q), gpu(f.b), gpu(f.users), gpu(f.full_indptr)[f.lead:], gpu(f.eval_items),
                             gpu(f.seen_indptr), gpu(f.seen_indices), ks=(5,), auc=True, masked_negatives=True,
                             per_user=True)
    got = per["auc"].cpu().numpy()
    assert got.dtype == np.float64
    with np.errstate(invalid="ignore"):
        want = wins.astype(np.float64) / (T.astype(np.float64) * n_neg.astype(np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= np.spacing(want[ok])).all(), (got, want)
