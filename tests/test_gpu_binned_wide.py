"""The split binned snapshot sort with 17-bit ids (k_sort_binned_split's WIDE form, 65,536 <= I <= 131,071 items:
Yelp's 92,090) against the oracle's stable descending order, and `Engine.refresh_info` — the observable that says
which sorter a refresh ran, without which every check below would pass on the radix route alone.

Shapes: the smallest tables at which a 17th id bit exists — 65,536 (the first wide size; its ids still fit 16
bits), 65,537 (one id with bit 16), Yelp's item count, 131,071 (the last size; G = 7) — at d = 4 and 8 columns."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = ["normal", "few-ties", "ties", "spike", "skewed", "equal"]


def close(a, b, tol):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def make_engine(P, Q):
    from revisit_bpr.engine import Engine

    return Engine(torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), None)


def tables(I, d, kind, rng):
    """tests/test_gpu_parity.py's _binned_tables (the kinds used here), plus ties planted ACROSS the 16-bit boundary:
    rows i and i + 65,536 equal — ids that differ in bit 16 only, which an id cut to 16 bits cannot tell apart."""
    Q = (rng.standard_normal((I, d)) * 0.05).astype(np.float32)
    if kind == "ties":          # a few dozen distinct values per column: bins overflow -> the radix fallback
        Q = (np.round(Q * 400) / 400).astype(np.float32)
    elif kind == "few-ties":    # birthday collisions and planted equal rows, +0 / -0
        Q[5] = Q[7]
        Q[I // 2] = Q[I // 2 + 3]
        Q[I - 1] = Q[1]
        Q[11] = 0.0
        Q[13] = -0.0
        Q[17] = 0.0
    elif kind == "spike":       # a trained model's cold items: most keys within a hair of zero, heavy tails
        cold = rng.random(I) < 0.7
        Q[cold] *= 1e-3
        Q[rng.integers(1, I, 20)] *= 40.0
    elif kind == "skewed":      # one-sided, exponential
        Q = (rng.exponential(0.05, (I, d))).astype(np.float32)
    elif kind == "equal":
        Q[:] = np.float32(0.25)
    Q[0] = 0
    for i in (0, 1, 2, 777, 12345, I - 65537):  # i = 0: the pad row's zeros; I - 65,537: the last row
        if 0 <= i and i + 65536 < I:
            Q[i + 65536] = Q[i]
    if I > 65536:
        Q[65535] = Q[65536]
    return Q


def plan_g(I):
    """bpr_refresh_plan.h: a stretch of I / G keys + 6 % + a 64-entry window must fit 20,480 staged entries."""
    g = (I * 106 // 100 + 20 * 1024 - 1) // (20 * 1024)
    while (I // g) * 106 // 100 + 64 > 20 * 1024:
        g += 1
    return g


@pytest.mark.parametrize("d", [4, 8])
@pytest.mark.parametrize("I", [65536, 65537, 92090, 131071])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_split_binned_sort_is_the_stable_descending_order(I, d, kind):
    """Bit-equal orders from the default engine, the radix route (`binned_sort` 0), the split binned sort forced at
    the plan's G and at G + 1, and the side-stream refresh (_begin + _commit); sigma within the project's 2e-6
    wherever the oracle's is positive.  On the forced engines `refresh_info` must name the split binned sort with the
    G asked for; `normal` columns never fall back (an average bin holds I / (G x 4,096) <= 5 keys against BIN_MAX =
    64), all-equal columns all do, heavily tied ones may."""
    rng = np.random.default_rng(I * 13 + d + len(kind))
    Q = tables(I, d, kind, rng)
    P = np.zeros((4, d), np.float32)
    QT, sigma_o = oracle.adaptive_stats(Q)
    order_o = oracle.adaptive_order(QT)
    G = plan_g(I)
    assert G * 20 * 1024 >= I * 1.06
    for name, tune in (("default", {}), ("radix", {"binned_sort": 0}), ("split", {"binned_split": G}),
                       ("split+1", {"binned_split": G + 1}), ("begin-commit", {})):
        e = make_engine(P, Q)
        for k, v in tune.items():
            e.set_tuning(k, v)
        if name == "begin-commit":
            e.adaptive_refresh_begin()
            e.adaptive_refresh_commit()
        else:
            e.adaptive_refresh()
        order, sigma = e.adaptive_snapshot()
        info = e.refresh_info()
        order = order.cpu().numpy()
        assert np.array_equal(order, order_o), (name, kind, int(np.argmax((order != order_o).any(axis=0))))
        pos = sigma_o > 0
        assert close(sigma.cpu().numpy()[pos], sigma_o[pos], 2e-6), (name, kind)
        if name == "radix":
            assert info["route"] == "radix" and info["g"] == 0 and info["fallback_columns"] is None
        if name.startswith("split"):
            want = G + (name == "split+1")
            assert info["route"] == "binned_split" and info["g"] == want, (name, info)
            assert info["items"] in (8, 12, 16, 20) and want * info["items"] * 1024 >= I * 1.06
            assert info["sub"] == 4  # the fallback's radix workgroups per column (d x sub < 256, pieces >= 5,000 keys)
            if kind == "normal":
                assert info["fallback_columns"] == 0
            elif kind == "equal":
                assert info["fallback_columns"] == d
            else:
                assert 0 <= info["fallback_columns"] <= d


def test_existing_split_range_reports_its_route():
    """MSD's 41,141 items: still the 16-bit split binned sort with G = 3 (41,141 x 1.06 / 20,480 -> 3) and SITEMS 16
    (13,713 x 1.06 + 64 = 14,599 <= 16,384), now visible through refresh_info."""
    I, d = 41141, 16
    rng = np.random.default_rng(41141)
    Q = tables(I, d, "normal", rng)
    P = np.zeros((4, d), np.float32)
    e = make_engine(P, Q)
    assert e.refresh_info()["route"] is None  # no refresh yet
    e.adaptive_refresh()
    info = e.refresh_info()
    assert info["route"] == "binned_split" and info["g"] == 3 and info["items"] == 16
    assert info["fallback_columns"] == 0
    assert np.array_equal(e.adaptive_snapshot()[0].cpu().numpy(), oracle.adaptive_order(oracle.adaptive_stats(Q)[0]))
