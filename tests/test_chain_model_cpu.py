"""tests/chain_model.py on the CPU: its fma against exact rational arithmetic, the IEEE identities the serving kernels
depend on, and the POWER of the GPU test built on it — on that test's own inputs another chain order, and a float64
matmul rounded once, give different bits in a large share of the pairs, so holding a kernel to the contract order's bits
is not vacuous.  No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

from chain_model import CONTRACT, NATURAL, F, bits, chain_scores, cosine_scores, fma32, rn, select, ss, value_tables

TWO = Fraction(2)


def round_to_float32(x: Fraction) -> np.float32:
    """x (finite, exact) -> the nearest float32, ties to even, subnormals included, overflow to inf; the sign of a zero
    result is the caller's business (an exact zero sum has IEEE's sign rules, not a rounding's)."""
    if x == 0:
        return F(0)
    sign, m = (-1 if x < 0 else 1), abs(x)
    e = m.numerator.bit_length() - m.denominator.bit_length()  # 2^(e-1) < m < 2^(e+1)
    if TWO ** e > m:
        e -= 1
    assert TWO ** e <= m < TWO ** (e + 1)
    q = max(e, -126) - 23  # the grid's spacing is 2^q: 24 bits, or the subnormals' 2^-149
    n = m / TWO ** q
    k = n.numerator // n.denominator
    r = n - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k & 1):
        k += 1
    v = Fraction(k) * TWO ** q
    if v >= TWO ** 128:
        return F(sign * np.inf)
    out = F(np.ldexp(float(k), q))  # (k < 2^25 and the result is on float32's grid: exact)
    assert Fraction(float(out)) == v
    return F(sign) * out


def exact_fma(a, b, c) -> np.float32:
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:  # exact zero: +0 unless both addends are negative zeros (round to nearest)
        prod_neg = np.signbit(a) != np.signbit(b)
        return F(-0.0) if prod_neg and np.signbit(c) and float(c) == 0 and float(a) * float(b) == 0 else F(0.0)
    r = round_to_float32(x)
    return F(-0.0) if r == 0 and x < 0 else r


def triples(kind, n, rng):
    g = lambda: rng.standard_normal(n)  # noqa: E731
    if kind == "ordinary":
        a, b, c = g(), g(), g()
    elif kind == "wide":
        a, b, c = (np.ldexp(g(), rng.integers(-20, 21, n)) for _ in range(3))
    elif kind == "subnormal":  # products around 2^-140, c around them, some far below and some exactly 0
        a, b = np.ldexp(g(), rng.integers(-80, -60, n)), np.ldexp(g(), rng.integers(-80, -60, n))
        c = np.ldexp(g(), rng.integers(-152, -125, n))
        c[::7] = 0.0
        c[3::7] = -0.0
    else:
        assert kind == "large_c"  # the product is a fraction of c's last bit: the double rounding's home
        a, b = g(), g()
        c = np.ldexp(g(), rng.integers(20, 60, n))
        # every second triple built like the one of test_fma32_at_the_constructed_double_rounding: a b = 4^j - 4^-t is
        # just below half of c's spacing 2^(2j+1), by less than float64 can keep next to c
        h = n // 2
        j = rng.integers(0, 4, h)
        t = rng.integers(15, 24 - j)
        sign = rng.choice([-1.0, 1.0], h)
        a[:h], b[:h] = sign * (2.0 ** j + 2.0 ** -t), 2.0 ** j - 2.0 ** -t
        c[:h] = sign * np.ldexp((2 ** 23 + rng.integers(0, 2 ** 23, h)).astype(np.float64), 2 * j + 1)
    return a.astype(F), b.astype(F), c.astype(F)


@pytest.mark.parametrize("kind", ["ordinary", "wide", "subnormal", "large_c"])
def test_fma32_is_the_exactly_rounded_fma(kind):
    rng = np.random.default_rng(len(kind))
    a, b, c = triples(kind, 3000, rng)
    got = fma32(a, b, c)
    assert got.dtype == F and got.shape == a.shape
    want = np.array([exact_fma(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if kind == "subnormal":  # what the class is there for
        tiny = np.abs(want) < F(2.0 ** -126)
        assert (tiny & (want != 0)).sum() > 500 and (want == 0).any()
    if kind == "large_c":    # the naive form is wrong somewhere here, or the class proves nothing
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
        print("naive double rounding differs in", int((naive != want).sum()), "of", len(want))
        assert (naive != want).sum() > 300


def test_fma32_at_the_constructed_double_rounding():
    a, b, c = F(8 + 2.0 ** -20), F(8 - 2.0 ** -20), F(2.0 ** 30 + 128)
    assert float(a) == 8 + 2.0 ** -20 and float(c) == 2.0 ** 30 + 128
    naive = F(np.float64(a) * np.float64(b) + np.float64(c))
    assert float(naive) == 2.0 ** 30 + 256          # rounds twice: up to the tie, then to even
    assert float(fma32(a, b, c)) == 2.0 ** 30 + 128  # 64 - 2^-40 is below half of the spacing 128
    assert fma32(a, b, c) == exact_fma(a, b, c)


def test_fma32_zeros_infinities_and_nans():
    inf, nan, tiny = F(np.inf), F(np.nan), F(2.0 ** -80)
    one = lambda a, b, c: fma32(F(a), F(b), F(c)).reshape(())[()]  # noqa: E731
    # a negative product that underflows onto +0 is -0 ...
    r = one(-tiny, tiny, 0.0)
    assert r == 0 and np.signbit(r)
    # ... and a staged zero after it makes +0 of it: why the padded zeros are run and not skipped
    r2 = one(0.0, 0.0, r)
    assert r2 == 0 and not np.signbit(r2)
    assert np.signbit(one(0.0, -0.0, -0.0)) and not np.signbit(one(0.0, 0.0, -0.0))
    assert not np.signbit(one(1.0, 1.0, -1.0))        # an exact cancellation is +0
    assert one(-tiny, tiny, 2.0 ** -149) == F(2.0 ** -149)  # far below half an ulp of the smallest subnormal
    assert one(2.0 ** -75, 2.0 ** -75, 0.0) == 0      # 2^-150: the tie goes to even, which is 0
    assert one(2.0 ** -75, 1.5 * 2.0 ** -75, 0.0) == F(2.0 ** -149)
    assert np.isnan(one(inf, 0.0, 1.0)) and np.isnan(one(0.0, inf, -inf)) and np.isnan(one(nan, 1.0, 1.0))
    assert np.isnan(one(inf, 1.0, -inf)) and np.isnan(one(1.0, 1.0, nan))
    assert one(inf, 2.0, 1.0) == inf and one(inf, -2.0, inf) != inf and one(-inf, 2.0, 5.0) == -inf
    assert one(1.0, 1.0, inf) == inf and one(1.0, 1.0, -inf) == -inf
    big = F(2.0 ** 100)
    assert one(big, big, 0.0) == inf and one(big, -big, 0.0) == -inf     # overflow
    assert one(big, big, -inf) == -inf                                    # (the product is finite before it is rounded)
    fmax = np.finfo(F).max
    assert one(fmax, 1.0, fmax * F(2.0 ** -25)) == fmax                   # just below the overflow threshold: stays finite
    assert one(fmax, 1.0, fmax * F(2.0 ** -24)) == inf
    v = fma32(np.array([1, 2], F)[:, None], np.array([3, 4, 5], F)[None, :], F(1))  # broadcasting
    assert v.shape == (2, 3) and np.array_equal(v, np.array([[4, 5, 6], [7, 9, 11]], F))


def test_chain_scores_is_the_contract():
    """the order, the padding and the bias, each shown by a table on which it matters"""
    rng = np.random.default_rng(1)
    for d in (1, 7, 8, 33, 64):
        A, B = rng.standard_normal((5, d)).astype(F), rng.standard_normal((6, d)).astype(F)
        bias = rng.standard_normal(6).astype(F)
        got = chain_scores(A, B, bias)
        assert got.dtype == F and got.shape == (5, 6)
        for i in range(5):
            for j in range(6):
                acc = F(0)
                for f8 in range(0, -(-d // 32) * 32, 8):
                    for o in (0, 4, 1, 5, 2, 6, 3, 7):
                        f = f8 + o
                        x, y = (A[i, f], B[j, f]) if f < d else (F(0), F(0))
                        acc = exact_fma(x, y, acc)
                assert bits(got[i, j]) == bits(acc + bias[j])
    # the padded zeros are run: d = 8 ends on -0 and the staged zeros of its chunk make +0 of it; d = 32 has none
    for d, neg in ((8, False), (32, True), (33, False), (64, True)):
        a, b = np.zeros((1, d), F), np.zeros((1, d), F)
        a[0, d - 1], b[0, d - 1] = -2.0 ** -80, 2.0 ** -80
        s = chain_scores(a, b)[0, 0]
        assert s == 0 and bool(np.signbit(s)) == neg, d
    # the bias is ONE add after the chain, not the chain's start: 2^24 + 1 + 1 is 2^24 one way and 2^24 + 2 the other
    a, b = np.ones((1, 2), F), np.ones((1, 2), F)
    assert chain_scores(a, b, np.array([2.0 ** 24], F))[0, 0] == F(2.0 ** 24 + 2)
    assert np.array_equal(ss(a), np.array([2], F)) and chain_scores(a, b, order=NATURAL)[0, 0] == 2


def test_cosine_pieces_and_select():
    T = np.array([[3, 4], [0, 0], [np.nan, 1], [2.0 ** 70, 2.0 ** 70], [np.inf, 0], [1, 0]], F)
    r = rn(ss(T))
    assert r[0] == F(0.2) and r[1] == -1 and r[2] == -1  # a zero row and a NaN row carry the marker ...
    assert r[3] == 0 and r[4] == 0 and not np.signbit(r[3])  # ... an ss that overflowed is +inf > 0: rn = +0
    S, ok_t, ok_x = cosine_scores(T[[0, 5]], T)
    assert ok_t.tolist() == [True, False, False, True, True, True] and ok_x.all()
    assert S[0, 0] == F(F(F(25) * F(0.2)) * F(0.2)) and S[0, 3] == 0 and np.isnan(S[0, 4]) and np.isnan(S[1, 4])
    # select: NaN never, -0 == +0 (the id decides), -inf real items keep their ids, then padding
    s = np.array([1, np.nan, -0.0, 0.0, -np.inf, np.inf, np.inf, -np.inf], F)
    ids, sc = select(s, np.arange(10, 18), 9)
    assert ids.tolist() == [15, 16, 10, 12, 13, 14, 17, -1, -1]
    assert np.signbit(sc[3:5]).tolist() == [True, False] and np.isneginf(sc[5:]).all()
    assert select(s, np.arange(10, 18), 2)[0].tolist() == [15, 16]


# ---- the power of tests/test_gpu_chain.py ------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["a", "b"])
@pytest.mark.parametrize("d", [7, 8, 33, 100, 128])
def test_another_order_changes_the_bits_of_the_gpu_tests_inputs(cls, d):
    """On the GPU test's tables (its U, I and seed rule), the natural order 0 .. 7 and a float64 matmul rounded once to
    float32 each differ from the contract order in at least 20 % of the pairs.  (d = 1 has one order.)"""
    from test_gpu_chain import I, U, seed_of

    P, Q, _ = value_tables(cls, U, I, d, seed_of(cls, d))
    want = chain_scores(P, Q)
    natural = chain_scores(P, Q, order=NATURAL)
    matmul = (P.astype(np.float64) @ Q.astype(np.float64).T).astype(F)
    share_n = float((bits(natural) != bits(want)).mean())
    share_m = float((bits(matmul) != bits(want)).mean())
    print(f"class {cls} d {d}: natural order differs in {share_n:.1%} of the pairs, float64 matmul in {share_m:.1%}")
    assert share_n >= 0.20 and share_m >= 0.20
    assert CONTRACT != NATURAL
