"""The serving kernels' score, restated exactly on the host: test infrastructure, nothing of it comes from the code
under test.  revisit-bpr_amd/csrc/bpr_topk_shared.h states the contract — ONE fp32 accumulator from +0, one fused
multiply-add per feature, per 8 features in the order 0, 4, 1, 5, 2, 6, 3, 7, every chunk of 32 features run to its end
over staged zeros, the bias one fp32 add afterwards — and this file is that sentence in numpy, with a correctly rounded
fma, so that a GPU test can hold the kernels' scores to it bit for bit (tests/test_gpu_chain.py) and a CPU test can
hold the fma to exact rational arithmetic (tests/test_chain_model_cpu.py).

Also here, because both of those tests need them: the cosine pieces of bpr_neighbors.hip, the result order as a
function (`select`), and the value classes the GPU test runs (`value_tables`)."""
import numpy as np

F = np.float32
CONTRACT = (0, 4, 1, 5, 2, 6, 3, 7)  # bpr_topk_shared.h: a lane half holds features 0 .. 3, the other 4 .. 7
NATURAL = (0, 1, 2, 3, 4, 5, 6, 7)   # what the contract is NOT (the CPU test's power check)
CHUNK = 32                           # TOPK_KC: a chain runs whole chunks


def fma32(a, b, c):
    """fl32(a * b + c), rounded once: the IEEE-754 fusedMultiplyAdd of float32, elementwise with broadcasting.

    The float64 product of two float32 is exact (24 + 24 bits, and no float32 product leaves float64's range).  The
    float64 sum p + c is not: TwoSum gives its rounding error, and where there is one the sum is moved onto the
    neighbour with an odd last bit (round to odd), which the final cast to float32 then rounds as if it had seen the
    exact sum (53 >= 24 + 2 bits; a subnormal result keeps fewer bits, which only helps).  The naive
    float32(float64(a) * b + c) rounds twice and is wrong at a = 8 + 2^-20, b = 8 - 2^-20, c = 2^30 + 128.
    Non-finite values and signed zeros are float64's, which are IEEE's: inf * 0 + c = NaN, a negative product that
    underflows onto +0 gives -0, and fma(0, 0, -0) = +0."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = np.atleast_1d(p + c64)
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)  # TwoSum: s + err == p + c exactly (where s is finite)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(inexact & even, odd, s).astype(F).reshape(a.shape)


def _chain(A, B, order, pairwise):
    """the chain over the features of A [n, d] and B [m, d]: every pair of rows ([n, m]) or row by row ([n], n == m)"""
    A, B = np.asarray(A, F), np.asarray(B, F)
    assert A.ndim == B.ndim == 2 and A.shape[1] == B.shape[1] and sorted(order) == list(range(8))
    d = A.shape[1]
    dpad = -(-d // CHUNK) * CHUNK
    Ap, Bp = np.zeros((A.shape[0], dpad), F), np.zeros((B.shape[0], dpad), F)  # zeros past d, on both sides
    Ap[:, :d], Bp[:, :d] = A, B
    acc = np.zeros((A.shape[0], B.shape[0]) if pairwise else A.shape[0], F)    # from +0
    for f8 in range(0, dpad, 8):
        for j in order:
            f = f8 + j
            acc = fma32(Ap[:, f][:, None], Bp[:, f][None, :], acc) if pairwise else fma32(Ap[:, f], Bp[:, f], acc)
    return acc


def chain_scores(P_rows, Q_rows, bias=None, order=CONTRACT):
    """s(u, i) for every pair of rows of P_rows [n, d] and Q_rows [m, d], float32 [n, m]: the chain, then `bias` [m]
    as one fp32 add.  `order`: the order inside every block of 8 features (the contract's, unless a test wants to
    see what another one would give)."""
    acc = _chain(P_rows, Q_rows, order, True)
    if bias is not None:
        with np.errstate(all="ignore"):
            acc = (acc + np.asarray(bias, F)[None, :]).astype(F)
    return acc


def ss(V, order=CONTRACT):
    """ss(v) = chain(v, v) for every row of V, float32 [n] (k_neighbors_norms: fma_chain8(lo, hi, lo, hi, ss))"""
    V = np.asarray(V, F)
    return _chain(V, V, order, False)


def rn(ssv):
    """bpr_neighbors.hip, k_neighbors_norms: `*dst = ss > 0.f ? 1.0f / sqrtf(ss) : -1.0f` — the correctly rounded
    square root, then the correctly rounded division (numpy's float32 arithmetic); the marker -1 for a zero row and
    for a NaN.  An ss that overflowed is +inf > 0: rn = +0, and the row stays eligible."""
    ssv = np.asarray(ssv, F)
    good = ssv > 0
    with np.errstate(all="ignore"):
        return np.where(good, F(1) / np.sqrt(np.where(good, ssv, F(1)), dtype=F), F(-1)).astype(F)


def cosine_scores(X_rows, T_rows):
    """(S [n, m] float32, ok_t [m], ok_x [n]).  S restates bpr_neighbors.hip, k_neighbors, step (A):
    `acc0[q] = __fmul_rn(__fmul_rn(acc0[q], rt), rx0)` — the dot product times the TABLE row's rn first, then times
    the query's.  ok_t: the table row is eligible (`rt >= 0.f`); ok_x: the query has a norm (`rx >= 0.f`), else its row
    of the result is all padding."""
    dot = chain_scores(X_rows, T_rows)
    rt, rx = rn(ss(T_rows)), rn(ss(X_rows))
    with np.errstate(all="ignore"):
        S = ((dot * rt[None, :]).astype(F) * rx[:, None]).astype(F)
    return S, rt >= 0, rx >= 0


def select(scores, ids, k):
    """The result order: of the candidates (scores [c] float32, ids [c]) the k best by score descending, then id
    ascending, -0 == +0; a NaN score is never returned; padded with (-inf, -1).  Returns (ids [k] int32, scores [k]
    float32); a returned score keeps its bits."""
    scores, ids = np.asarray(scores, F), np.asarray(ids, np.int64)
    keep = ~np.isnan(scores)
    scores, ids = scores[keep], ids[keep]
    top = np.lexsort((ids, -scores.astype(np.float64)))[:k]  # (comparisons: -0.0 == 0.0, -inf last)
    out_i, out_s = np.full(k, -1, np.int32), np.full(k, -np.inf, F)
    out_i[:len(top)], out_s[:len(top)] = ids[top], scores[top]
    return out_i, out_s


def select_rows(S, ok, k):
    """`select` per row of S [n, m] over the columns where ok [n, m]: (ids [n, k], scores [n, k])"""
    cols = np.arange(S.shape[1])
    rows = [select(S[r, ok[r]], cols[ok[r]], k) for r in range(S.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def bits(x):
    """float32 -> int32 bit patterns, every NaN as ONE pattern: IEEE leaves the sign and payload of a NaN that an
    operation makes to the implementation, and x86 and gfx950 choose differently.  Everything else keeps its bits,
    the sign of a zero included."""
    x = np.ascontiguousarray(x, F)
    return np.where(np.isnan(x), np.int32(0x7FC00000), x.view(np.int32))


# ---- the value classes of tests/test_gpu_chain.py (here, so that the CPU test measures the model's power on them) ----
def value_tables(cls, U, I, d, seed):
    """(P [U, d], Q [I, d], b [I]) float32 of value class `cls`, without the special rows the GPU test adds:
    "a" ordinary, randn; "b" wide range, randn * 2^randint(-12, 12): heavy cancellation, sensitive to the order;
    "c" subnormal, class (a) times 2^-68: products and partial sums between 2^-149 and 2^-126, some below;
    "d" non-finite: class (a), to which the GPU test adds its infinities and NaNs."""
    rng = np.random.default_rng(seed)
    P, Q = rng.standard_normal((U, d)).astype(F), rng.standard_normal((I, d)).astype(F)
    b = rng.standard_normal(I).astype(F)
    if cls == "b":
        P = np.ldexp(P, rng.integers(-12, 13, P.shape)).astype(F)
        Q = np.ldexp(Q, rng.integers(-12, 13, Q.shape)).astype(F)
        b = np.ldexp(b, rng.integers(-12, 13, b.shape)).astype(F)
    elif cls == "c":
        P, Q, b = np.ldexp(P, -68).astype(F), np.ldexp(Q, -68).astype(F), np.ldexp(b, -136).astype(F)
    else:
        assert cls in "ad"
    return P, Q, b
