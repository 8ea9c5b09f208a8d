"""The yardstick of the ROC-AUC tests, on a machine without a GPU: the all-pairs model (tests/auc_model.py) against
oracle/metrics_np.py and the product's dense RocAucMany — neither is the code under test on the GPU —, then the
product's sort-based RocAucManySlow and `evaluate_topk(auc=True)` on CPU tensors against the model, NaN scores
included, and the float32 resolution argument that tests/test_gpu_auc.py rests on.

Rows: tests/auc_cases.py (I <= 64, every T from 1 to I, multiples of 1 / 2 with -1e13, +-inf, +-0 and subnormals).
The rows are so small that T (I - T) <= 1,024: every quotient below is a correctly rounded float32 division of two
small integers in each of the forms compared, so "the same counts" is "the same float32 bits", and the count is read
back from the value as round(value * T * n_neg)."""
import numpy as np
import pytest

from auc_cases import MIXED_I, TN_MAX, boundary_shapes, family, nan_rows, one_user, small_rows, whole_call
from auc_model import auc_row, auc_rows, bits, value_of

torch = pytest.importorskip("torch")


def dense(rows):
    """[(scores, ids)] of one width -> (output [n, I], target [n, I]) float32."""
    out = np.stack([s for s, _ in rows])
    target = np.zeros_like(out)
    for r, (_, t) in enumerate(rows):
        target[r, t] = 1.0
    return out, target


def by_width(rows):
    widths = {}
    for s, t in rows:
        widths.setdefault(len(s), []).append((s, t))
    return widths.values()


def check(got, rows):
    """float32 values of a dense form against the model: bits, and the integer count behind them."""
    for g, (s, t) in zip(np.asarray(got, np.float32), rows):
        wins, T, n_neg, value = auc_row(s, t)
        assert bits(g) == bits(value), (len(s), T, wins, float(g), float(value))
        if T * n_neg:
            assert round(float(g) * T * n_neg) == wins and abs(float(g) * T * n_neg - wins) < 1e-3


def test_the_rows_hold_what_they_are_there_for():
    rows = small_rows()
    assert {(len(s), len(t)) for s, t in rows} >= {(I, T) for I in (1, 2, 64) for T in range(1, I + 1)}
    flat = np.concatenate([s for s, _ in rows])
    assert np.isposinf(flat).any() and np.isneginf(flat).any() and (flat == np.float32(-1e13)).any()
    assert (np.signbit(flat) & (flat == 0)).any() and (~np.signbit(flat) & (flat == 0)).any()
    assert ((np.abs(flat) < np.float32(2.0 ** -126)) & (flat != 0)).any()
    assert not np.isnan(flat).any()
    ties = sum(bool((s[t][:, None] == np.delete(s, t)[None, :]).any()) for s, t in rows)
    assert ties > 50  # rows in which '>' and '>=' count differently
    kinds = {k % 4 for k, (s, _) in enumerate(rows) if len(s) >= 3}
    assert kinds == {0, 1, 2, 3} and all(np.isnan(s).any() or len(t) == len(s) for s, t in nan_rows(rows))


def test_model_by_hand():
    s = np.array([0.0, -0.0, 2.0 ** -149, 0.0, -(2.0 ** -149), np.inf, -np.inf, np.nan], np.float32)
    # +0 beats -2^-149 and -inf; the subnormal beats -0, 0, -2^-149 and -inf; nothing beats or is beaten by NaN
    assert auc_row(s, [0, 2])[:3] == (6, 2, 6)
    assert auc_row(s, [2, 0, 2, 0])[:3] == (6, 2, 6)  # a set
    assert auc_row(s, [7])[:3] == (0, 1, 7) and auc_row(s, [7])[3] == 0.0
    assert auc_row(s, [5])[:3] == (6, 1, 7)  # +inf beats all but NaN
    assert auc_row(s, [6])[:3] == (0, 1, 7)
    assert auc_row(np.array([1, 0, 0], np.float32), [0, 0])[:3] == (2, 1, 2)
    assert auc_row(np.array([1, 0, 0], np.float32), [0, 0])[3] == 1.0
    assert auc_row(np.array([1, np.nan, 0, 0.5], np.float32), [0])[3] == np.float32(2 / 3)
    assert np.isnan(auc_row(s, [])[3]) and np.isnan(auc_row(s, range(8))[3])  # T = 0, T = I
    many = np.zeros(5000, np.float32)
    assert np.isnan(auc_row(many, range(4097))[3]) and auc_row(many, range(4097), t_max=None)[3] == 0.0
    assert auc_row(many, range(4096))[3] == 0.0
    w, T, n, v = auc_rows(np.stack([s, s]), np.array([3, 5, 6]), np.array([9, 9, 9, 0, 2, 5]))  # indptr from 3
    assert (w.tolist(), T.tolist(), n.tolist()) == ([6, 6], [2, 1], [6, 7]) and v[0] == np.float32(0.5)


def test_model_equals_the_oracle_and_the_dense_class():
    from oracle import metrics_np
    from revisit_bpr.metrics.auc import RocAucMany

    for rows in by_width(small_rows()):
        out, target = dense(rows)
        with np.errstate(invalid="ignore"):
            check(metrics_np.roc_auc_many(out, target), rows)
        check(RocAucMany().compute(torch.from_numpy(out), torch.from_numpy(target)).numpy(), rows)


def test_sort_based_class_equals_the_model_with_nan_scores_too():
    from revisit_bpr.metrics.auc import RocAucMany, RocAucManySlow

    plain = small_rows()
    for rows in list(by_width(plain)) + list(by_width(nan_rows(plain))):
        out, target = dense(rows)
        to, tt = torch.from_numpy(out), torch.from_numpy(target)
        check(RocAucManySlow().compute(to, tt).numpy(), rows)
        check(RocAucMany().compute(to, tt).numpy(), rows)  # (the dense class: pairwise '>', NaN and all)


def test_sort_based_class_with_a_mask_and_nan():
    """The mask argument (entries that are neither positives nor negatives) next to NaN scores."""
    from revisit_bpr.metrics.auc import RocAucManySlow

    s = np.array([[1.0, np.nan, 0.0, 0.5, np.nan, 2.0, -1.0]], np.float32)
    t = np.array([[1, 0, 0, 0, 1, 0, 0]], np.float32)
    m = np.array([[1, 1, 1, 1, 1, 0, 1]], np.float32)
    got = RocAucManySlow().compute(torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(m)).numpy()
    assert got[0] == np.float32(3 / (2 * 4))  # 1.0 beats 0, 0.5 and -1; not NaN; 2.0 is masked out


def test_evaluate_topk_on_cpu_tensors_equals_the_model():
    f = family()
    value = f.model[3]
    for e in range(f.E):
        got = one_user(f, e, "cpu")
        assert bits(got) == bits(value[e]), (e, float(got), float(value[e]), f.model[0][e], f.model[1][e])
    assert np.isnan(value[f.NO_TARGET]) and np.isnan(whole_call(f, (0, f.E), "cpu"))
    E = f.E - 1  # the users that have targets; blocks of 7 end inside them
    got = whole_call(f, (1, f.E), "cpu")
    want = float(np.mean(value[1:].astype(np.float64)))
    print("auc", got, "model", want, "bound", (E + 1) * 2.0 ** -24)
    assert abs(got - want) <= (E + 1) * 2.0 ** -24


def collisions(TN, w):
    a = (w / np.float64(TN)).astype(np.float32)
    b = ((w + 1) / np.float64(TN)).astype(np.float32)
    return int((a == b).sum())


def test_one_pair_changes_the_float32_up_to_2_pow_24():
    """float32(w / TN) != float32((w + 1) / TN) for every w in [0, TN) when TN <= 2^24: values lie in [0, 1], where
    float32 is spaced at most 2^-24 apart, and one pair moves the quotient by 1 / TN >= 2^-24.  Exhaustive at 2^24 and
    at the largest T (I - T) of the GPU file's shapes; beyond 2^24 it fails, at the (5, 9000, 5000) shape of the older
    test for one."""
    largest = max(max(T * (I - T) for T, I in boundary_shapes()), 4096 * (MIXED_I - 4096))
    assert largest == TN_MAX == 2 ** 24
    for TN in sorted({TN_MAX, largest, 4095 * 4096, 1023 * 257}):
        for lo in range(0, TN, 1 << 21):
            w = np.arange(lo, min(lo + (1 << 21), TN), dtype=np.float64)
            assert collisions(TN, w) == 0, (TN, lo)
    assert value_of(TN_MAX - 1, 4096, 4096) != value_of(TN_MAX, 4096, 4096) == 1.0
    TN = 4096 * 4904
    w = np.random.default_rng(0).integers(0, TN, 200_000).astype(np.float64)
    n = collisions(TN, w)
    print("collisions at TN = 4096 * 4904:", n, "of 200000")
    assert n > 0  # a miscounted pair can pass unnoticed there
