"""64-bit Philox counters and seeds on the CPU: the anchor of the oracle and the power of the GPU comparisons.

tests/test_gpu_counter64.py holds every sampling kernel to the oracle at counters whose high word is non-zero and at
a seed whose high word is non-zero.  Two things must hold for that to mean anything, and both are checked here without
a GPU:

  * the oracle itself splits counter and seed as documented (`bpr_device.h`: counter words (lo, hi, block, purpose),
    key words (lo, hi)): its picks are recomputed from `oracle.philox4x32_10` with the words formed in Python integers
    — so the oracle and the kernels cannot be wrong in the same way;
  * on the inputs of every GPU case, the stream a broken counter would draw (high word dropped; carry not propagated)
    differs from the right one in at least 90 % of the positions it affects.
"""
import math

import numpy as np
import pytest

import counter64_cases as cc
import oracle

SEED, M32 = cc.SEED, cc.M32
KEY = (SEED & M32, SEED >> 32)


def words(t, purpose):
    return oracle.philox4x32_10((t & M32, t >> 32, 0, purpose), KEY)


def test_the_seed_and_the_offsets_are_what_they_are_meant_to_be():
    assert SEED >> 63 == 1 and SEED >> 32 != 0 and SEED < 2 ** 64
    n = 20_000
    assert cc.offset_of("carry", n) == 2 ** 32 - n // 2 + 3
    assert cc.offset_of("rank1", n) == (1 << 40) + 12345
    assert cc.offset_of("rank7_carry", n) == (7 << 40) + 2 ** 32 - n // 2 + 3
    for name, wraps in (("carry", True), ("rank1", False), ("rank7_carry", True)):
        off = cc.offset_of(name, n)
        w = cc.wrap_of(off, n)
        assert (w < n) == wraps
        if wraps:  # off every run (1..8), group, wave (64) and batch (32, 256) boundary
            assert w == n // 2 - 3 and all(w % k for k in (2, 3, 4, 5, 6, 7, 8, 32, 64, 256))
            assert (off + w - 1) >> 32 == (off >> 32) and (off + w) >> 32 == (off >> 32) + 1 and (off + w) & M32 == 0


# ---- the oracle's own counter arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.OFFSETS)
def test_oracle_uniform_pick_is_the_documented_function_of_the_64_bit_counter(name):
    """Users with nothing seen accept their first candidate: pick = 1 + mulhi32(word 0 of block 0, I - 1)."""
    U, I, n = 50, 700, 64
    indptr, indices = np.zeros(U + 1, np.int64), np.zeros(0, np.int32)
    users = np.random.default_rng(1).integers(1, U, n).astype(np.int32)
    off = cc.offset_of(name, n)
    got = oracle.sample_uniform(indptr, indices, I, users, SEED, off)
    want = [1 + ((words(off + b, 0)[0] * (I - 1)) >> 32) for b in range(n)]
    assert got.tolist() == want
    if name != "rank1":
        assert (off >> 32) != ((off + n - 1) >> 32)  # across the wrap


@pytest.mark.parametrize("name", cc.OFFSETS)
def test_oracle_adaptive_draws_are_the_documented_function_of_the_64_bit_counter(name):
    """Factor: inverse CDF of |p_f| sigma_f in the lane-by-lane enumeration at threshold uf = (word 0 >> 8) / 2^24 of
    the purpose-1 block; rank: ceil(ln(ug) / ln(1 - p)), ug = ((word 1 >> 8) + 1) / 2^24, oriented by the sign of
    p_f.  The factor is recomputed exactly (the same double sums); the rank in double, and a draw whose
    ln(ug) / ln(1 - p) lies within fp32 rounding of an integer (4 ulp, the margin of
    test_adaptive_mismatches_are_cdf_bin_edges_and_ceil_flips) may take either neighbour."""
    U, I, d, n, p = 30, 400, 32, 64, 0.05
    rng = np.random.default_rng(2)
    P = rng.normal(0, 0.3, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.3, (I, d)).astype(np.float32)
    Q[0] = 0
    indptr, indices = np.zeros(U + 1, np.int64), np.zeros(0, np.int32)
    users = rng.integers(1, U, n).astype(np.int32)
    QT, sigma = oracle.adaptive_stats(Q)
    order = oracle.adaptive_order(QT)
    off = cc.offset_of(name, n)
    neg, fac, rnk = oracle.sample_adaptive(P, sigma, order, indptr, indices, users, p, SEED, off)
    G = 32
    enum = [f for lane in range(G) for f in range(lane, d, G)]
    n_unseen = I - 1
    for b in range(n):
        rf, rg = words(off + b, 1)[:2]
        w = (np.abs(P[users[b]]) * sigma).astype(np.float32)  # fp32 products, as the oracle forms them
        cum = np.cumsum(w[enum].astype(np.float64))
        thr = float(np.float32(rf >> 8) * np.float32(1.0 / 16777216.0)) * float(np.float32(cum[-1]))
        f = enum[int(np.nonzero(cum > thr)[0][0])]
        assert fac[b] == f, (b, fac[b], f)
        ug = float(np.float32((rg >> 8) + 1) * np.float32(1.0 / 16777216.0))
        x = math.log(ug) / math.log1p(-p)
        near = abs(x - round(x)) <= 4e-7 * max(1.0, abs(x)) * 4
        ranks = {max(1, min(n_unseen, r)) for r in ({math.ceil(x)} | ({round(x), round(x) + 1} if near else set()))}
        want = {r - 1 if P[users[b], f] > 0 else n_unseen - r for r in ranks}
        assert int(rnk[b]) in want, (b, rnk[b], want, x)
        assert neg[b] == oracle.adaptive_pick(order, indptr, indices, int(users[b]), int(fac[b]), int(rnk[b]))


# ---- the power of the GPU comparisons --------------------------------------------------------------------------------
def power(draw, users, names, n_wrap=None):
    """Share of positions in which a broken counter's stream differs from the right one, per (offset, way of
    breaking it), at the offsets the GPU case runs."""
    n = len(users)
    shares = {}
    for name in names:
        off = cc.offset_of(name, n, n_wrap)
        right = draw(users, off)
        for way, (wrong, where) in cc.wrong_streams(draw, users, off).items():
            assert where.stop - where.start >= 50, (name, way)
            shares[(name, way)] = float((wrong[where] != right[where]).mean())
    return shares


def uniform_draw(pr, **kw):
    return lambda users, off: cc.uniform(pr, users, off, **kw)


def adaptive_draw(pr):
    return lambda users, off: cc.adaptive(pr, users, off)[0]


# case: (inputs, the offsets its GPU tests run, the number of (offset, way) pairs that gives)
LDS = ("carry", "rank7_carry")
CASES = {
    "stream-32": (lambda: cc.stream_problem(32), cc.OFFSETS, 5), "stream-128": (lambda: cc.stream_problem(128), cc.OFFSETS, 5),
    "stream-256": (lambda: cc.stream_problem(256), cc.OFFSETS, 5), "lds-32": (lambda: cc.stream_problem(32, True), LDS, 4),
    "lds-128": (lambda: cc.stream_problem(128, True), LDS, 4), "lds-256": (lambda: cc.stream_problem(256, True), LDS, 4),
    "sequential-256": (cc.seq_problem, ("rank7_carry",), 2),
    "batched-sequential-64": (lambda: cc.synthetic_problem(64, 1500), ("carry",), 2),
    "batched-full-128": (cc.vstream_full_problem, ("rank1",), 1),
    "strict-64": (lambda: cc.synthetic_problem(64, 2000), ("carry",), 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_broken_counter_changes_the_picks_of_every_stream_case(case):
    """(Frozen tables: the adaptive picks of the cases that learn are those of their initial tables.  The planned
    cases walk the same users in another order; the share does not depend on the order.)"""
    make, names, pairs = CASES[case]
    pr = make()
    users = pr["users"]
    for kind, draw in (("uniform", uniform_draw(pr)), ("adaptive", adaptive_draw(pr))):
        if case.startswith("strict") and kind == "adaptive":
            continue
        shares = power(draw, users, names)
        print(case, kind, {"/".join(k): round(v, 4) for k, v in shares.items()})
        assert min(shares.values()) >= 0.9, (kind, shares)
        assert len(shares) == pairs  # carry offsets: both ways; rank1: the dropped high word


FOLD = ("carry", "rank1")


@pytest.mark.parametrize("d", [32, 128, 256])
def test_a_broken_counter_changes_the_picks_of_the_fold_in_cases(d):
    """The wrap falls inside the second epoch: the counter runs on over epochs x nnz."""
    pr = cc.foldin_problem(d)
    nnz = pr["nnz"]
    for kind, epochs, draw in (("uniform", cc.FOLD_EPOCHS, uniform_draw(pr)),
                               ("adaptive", cc.FOLD_ADAPTIVE_EPOCHS, adaptive_draw(pr))):
        shares = power(draw, np.tile(pr["users_of"], epochs), FOLD, n_wrap=nnz + nnz // 2 - 3)
        print("fold_in", d, kind, {"/".join(k): round(v, 4) for k, v in shares.items()})
        assert min(shares.values()) >= 0.9, (kind, shares)
    pr = cc.foldin_items_problem(d)
    nnz = pr["nnz"]
    shares = power(uniform_draw(pr), np.tile(pr["users"], cc.FOLD_EPOCHS), FOLD, n_wrap=nnz + nnz // 2 - 3)
    print("fold_in_items", d, {"/".join(k): round(v, 4) for k, v in shares.items()})
    assert min(shares.values()) >= 0.9, shares
