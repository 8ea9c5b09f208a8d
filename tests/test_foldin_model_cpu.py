"""The pipeline of `k_foldin` as a control-flow model (tests/foldin_model.py) against the definition: for every
prefetch depth, one or two groups in lockstep and any hand-out order, the rows come out bit for bit as the plain loop
over triples gives them.  The GPU tests run the one depth that is built; this holds the structure for all of them."""
import numpy as np
import pytest

from foldin_model import pipeline, restate

I, EPOCHS = 50, 3
LENGTHS = [0, 1, 2, 3, 9, 17, 40, 49]  # 49: every item seen, all negatives 0; 40 and 49 outlast every depth below


def inputs(seed=7, d=8, base=0):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)) for k in LENGTHS]
    indptr = base + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    items = np.concatenate([np.zeros(base, np.int64)] + rows).astype(np.int32)  # (base > 0: a slice of a larger CSR)
    neg = []
    for _ in range(EPOCHS):
        for row in rows:
            unseen = np.setdiff1d(np.arange(1, I), row)
            neg.append(rng.choice(unseen, size=len(row)) if len(unseen) else np.zeros(len(row), np.int64))
    Q = rng.normal(0, 0.5, (I, d))
    Q[0] = 0
    return Q, indptr, items, np.concatenate(neg).astype(np.int32), rng.normal(0, 0.1, (len(LENGTHS), d))


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4, 8])
def test_pipeline_applies_the_definition_bit_for_bit(pf, groups):
    Q, indptr, items, neg, P0 = inputs()
    want = restate(Q, indptr, items, neg, P0, EPOCHS, 0.05, 0.05)
    assert not np.array_equal(want[1:7], P0[1:7]) and np.array_equal(want[[0, 7]], P0[[0, 7]])
    n = len(LENGTHS)
    for order in (None, list(range(n))[::-1], list(np.random.default_rng(pf).permutation(n))):
        got, steps = pipeline(Q, indptr, items, neg, P0, EPOCHS, 0.05, 0.05, pf, groups, order)
        assert np.array_equal(got, want), (pf, groups, order)
        # a row costs its triples + 2 pf steps of fill and drain, + at most pf - 1 idle steps to ring slot 0
        rows_with_triples = sum(1 for k in LENGTHS if k)
        assert steps <= EPOCHS * sum(LENGTHS) + rows_with_triples * (3 * pf - 1)


def test_pipeline_on_a_slice_of_a_larger_csr_and_with_bad_ids():
    Q, indptr, items, neg, P0 = inputs(base=5)
    want = restate(Q, indptr, items, neg, P0, EPOCHS, 0.05, 0.0)
    got, _ = pipeline(Q, indptr, items, neg, P0, EPOCHS, 0.05, 0.0, 2, 2)
    assert np.array_equal(got, want)
    # an order entry out of range is passed over; a negative out of range skips its triple, as 0 does
    order = [7, 99, 6, 5, -1, 4, 3, 2, 1, 0][:len(LENGTHS)]
    got, _ = pipeline(Q, indptr, items, neg, P0, EPOCHS, 0.05, 0.0, 2, 2, order)
    kept = [r for r in order if 0 <= r < len(LENGTHS)]
    assert np.array_equal(got[kept], want[kept])
    untouched = [r for r in range(len(LENGTHS)) if r not in kept]
    assert np.array_equal(got[untouched], P0[untouched])
    bad = neg.copy()
    bad[bad == bad[bad > 0][0]] = I + 3
    zero = np.where(bad == I + 3, 0, bad).astype(np.int32)
    got, _ = pipeline(Q, indptr, items, bad, P0, EPOCHS, 0.05, 0.0, 4, 2)
    assert np.array_equal(got, restate(Q, indptr, items, zero, P0, EPOCHS, 0.05, 0.0))
