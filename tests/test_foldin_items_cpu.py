"""Item fold-in (`bpr_fold_in_item_rows`, revisit_bpr/foldin_items.py) on a machine without a GPU: the argument
validation of the entry point (nothing touches the device before the arguments are checked), the Python wrapper's
refusals, and the control-flow model of the kernel's four-stage pipeline (tests/foldin_items_model.py) against the
definition.  The launch layout is `plan_foldin`'s, which tests/test_foldin_cpu.py pins."""
import numpy as np
import pytest

from foldin_items_model import pipeline, restate

INVALID, UNSUPPORTED = -1, -3
GIVEN, UNIFORM, ADAPTIVE = 0, 1, 2


def lib():
    from revisit_bpr import native

    return native.load()


def rows(P=1, U=40, Q=1, bias=None, I=100, d=8, seen_indptr=None, seen_indices=None, indptr=1, users=1, m=4,
         order=None, epochs=3, lr=0.05, alpha=0.0, sampler=UNIFORM, neg_in=None, neg_out=None, Q_new=1,
         bias_new=None):
    """bpr_fold_in_item_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be
    refused before the device is touched, or m = 0, go through here."""
    return lib().bpr_fold_in_item_rows(P, U, Q, bias, I, d, seen_indptr, seen_indices, indptr, users, m, order, epochs,
                                       lr, alpha, sampler, neg_in, neg_out, 0, 0, Q_new, bias_new, None)


@pytest.mark.parametrize("kw, status, word", [
    (dict(d=0), INVALID, b"d must be"), (dict(d=1025), UNSUPPORTED, b"1024"), (dict(epochs=0), INVALID, b"epochs"),
    (dict(epochs=-3), INVALID, b"epochs"), (dict(sampler=ADAPTIVE), UNSUPPORTED, b"adaptive"),
    (dict(sampler=7), INVALID, b"sampler"), (dict(sampler=-1), INVALID, b"sampler"),
    (dict(lr=float("nan")), INVALID, b"NaN"), (dict(alpha=float("nan")), INVALID, b"NaN"),
    (dict(sampler=GIVEN, neg_in=None), INVALID, b"neg_in"),
    (dict(bias=1), INVALID, b"bias_new"), (dict(bias_new=1), INVALID, b"bias_new"),  # half-given bias pair
    (dict(seen_indptr=1), INVALID, b"seen_indices"), (dict(seen_indices=1), INVALID, b"seen_indices"),
    (dict(U=2 ** 21, d=1024), UNSUPPORTED, b"U * d"), (dict(I=2 ** 21, d=1024), UNSUPPORTED, b"I * d"),
    (dict(U=0), INVALID, b"U must be"), (dict(I=0), INVALID, b"I must be"), (dict(m=-1), INVALID, b"m must be"),
    (dict(m=2 ** 31), INVALID, b"2^31"), (dict(P=None), INVALID, b"NULL"), (dict(Q=None), INVALID, b"NULL"),
    (dict(indptr=None), INVALID, b"NULL"), (dict(users=None), INVALID, b"NULL"), (dict(Q_new=None), INVALID, b"NULL"),
])
def test_bad_arguments_are_refused_without_a_device(kw, status, word):
    assert rows(**kw) == status
    err = lib().bpr_last_error()
    assert b"bpr_fold_in_item_rows" in err and word in err, err


def test_no_rows_is_ok_without_tables():
    none = dict(P=None, Q=None, indptr=None, users=None, Q_new=None, m=0)
    assert rows(**none) == 0
    assert rows(**none, sampler=GIVEN) == 0
    assert rows(**none, epochs=0) == INVALID  # (still validated)
    assert rows(**none, d=1025) == UNSUPPORTED
    assert rows(**none, bias=1) == INVALID


def wrapper_inputs():
    import torch

    return dict(P=torch.zeros(5, 8), Q=torch.zeros(6, 8), item_bias=None,
                indptr=torch.tensor([0, 2, 3], dtype=torch.int64), users=torch.tensor([1, 4, 2], dtype=torch.int32),
                epochs=2, lr=0.05)


def call(args):
    from revisit_bpr.foldin_items import fold_in_items

    args = dict(args)
    return fold_in_items(args.pop("P"), args.pop("Q"), args.pop("item_bias"), args.pop("indptr"), args.pop("users"),
                         **args)


def test_wrapper_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    import revisit_bpr
    from revisit_bpr.foldin_items import fold_in_items

    assert revisit_bpr.fold_in_items is fold_in_items
    with pytest.raises(RuntimeError, match="ROCm"):
        call(wrapper_inputs())
    with pytest.raises(RuntimeError, match="ROCm"):
        call(dict(wrapper_inputs(), item_bias=torch.zeros(6), neg=torch.ones(6, dtype=torch.int32),
                  seen_indptr=torch.zeros(6, dtype=torch.int64), seen_indices=torch.zeros(0, dtype=torch.int32),
                  init=torch.zeros(2, 8), init_bias=torch.zeros(2)))


def test_wrapper_refuses_wrong_dtypes_and_lengths():
    torch = pytest.importorskip("torch")
    ok = wrapper_inputs()
    i64, i32 = torch.int64, torch.int32
    for bad in (dict(Q=ok["Q"].double()), dict(P=ok["P"].double()), dict(P=torch.zeros(5, 4)), dict(P=torch.zeros(5)),
                dict(Q=torch.zeros(6)), dict(indptr=ok["indptr"].int()), dict(users=ok["users"].long()),
                dict(item_bias=torch.zeros(5)), dict(item_bias=torch.zeros(6, dtype=torch.float64)),
                dict(indptr=torch.tensor([0, 2, 4], dtype=i64)),  # rows past the end of `users`
                dict(indptr=torch.tensor([2, 1], dtype=i64)), dict(indptr=torch.zeros(0, dtype=i64)),
                dict(neg=torch.ones(5, dtype=i32)), dict(neg=torch.ones(7, dtype=i32)), dict(neg=torch.ones(6, dtype=i64)),
                dict(init=torch.zeros(3, 8)), dict(init=torch.zeros(2, 4)), dict(init=torch.zeros(2, 8, dtype=torch.float64)),
                dict(init_bias=torch.zeros(2)),  # no item_bias to go with it
                dict(item_bias=torch.zeros(6), init_bias=torch.zeros(3)),
                dict(seen_indptr=torch.zeros(6, dtype=i64)), dict(seen_indices=torch.zeros(0, dtype=i32)),
                dict(seen_indptr=torch.zeros(5, dtype=i64), seen_indices=torch.zeros(0, dtype=i32)),  # not U + 1
                dict(seen_indptr=torch.zeros(6, dtype=i32), seen_indices=torch.zeros(0, dtype=i32)),
                dict(seen_indptr=torch.zeros(6, dtype=i64), seen_indices=torch.zeros(0, dtype=i64)),
                dict(epochs=0)):
        with pytest.raises(ValueError):
            call(dict(ok, **bad))


# ---- the control-flow model ------------------------------------------------------------------------------------------
U, I, EPOCHS = 40, 50, 3
# A row drains through 3 pf further steps: 3, 6, 12 at pf 1, 2, 4.  Rows of 1, 2 and 4 users make 3 epochs x length =
# exactly 3, 6 and 12 triples, rows of 6 and 12 users have exactly a drain's length; the others are shorter or longer.
LENGTHS = [0, 1, 2, 3, 4, 6, 9, 12, 17, 33, 40]
SEEN_LENGTHS = [0, 1, 17, 48, 49] + [5] * (U - 5)  # user 3 has seen all but item 23, user 4 every item


def inputs(seed=7, d=8, base=0):
    rng = np.random.default_rng(seed)
    audience = [np.sort(rng.choice(U, size=k, replace=False)) for k in LENGTHS]
    indptr = base + np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    users = np.concatenate([np.zeros(base, np.int64)] + audience).astype(np.int32)  # (base > 0: a slice of a larger CSR)
    srows = [np.setdiff1d(np.arange(1, I), [23]) if k == 48 else np.sort(rng.choice(np.arange(1, I), size=k, replace=False))
             for k in SEEN_LENGTHS]
    seen = (np.concatenate([[0], np.cumsum(SEEN_LENGTHS)]).astype(np.int64), np.concatenate(srows).astype(np.int64))
    neg = rng.integers(1, I, EPOCHS * sum(LENGTHS)).astype(np.int32)
    neg[::11] = 0  # some triples are skipped
    P = rng.normal(0, 0.5, (U, d))
    Q = rng.normal(0, 0.5, (I, d))
    Q[0] = 0
    m = len(LENGTHS)
    return dict(P=P, Q=Q, bias=rng.normal(0, 0.5, I), indptr=indptr, users=users, neg=neg, seen=seen,
                Q0=rng.normal(0, 0.1, (m, d)), b0=rng.normal(0, 0.1, m))


def draw(u, seen_row, t):
    """A stand-in for the device sampler: a pure function of (the user's seen row, the counter)."""
    unseen = np.setdiff1d(np.arange(1, I), seen_row)
    return int(unseen[(t * 2654435761 + 12345) % len(unseen)]) if len(unseen) else 0


def run(x, neg, bias, pf, groups, order=None, seen=None, reg=0.05):
    b = x["bias"] if bias else None
    want = restate(x["P"], x["Q"], b, x["indptr"], x["users"], neg, x["Q0"], x["b0"], EPOCHS, 0.05, reg, seen=seen)
    got = pipeline(x["P"], x["Q"], b, x["indptr"], x["users"], neg, x["Q0"], x["b0"], EPOCHS, 0.05, reg, pf, groups,
                   order, seen=seen)
    return want, got


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_applies_the_definition_bit_for_bit(pf, groups, bias):
    x = inputs()
    m = len(LENGTHS)
    for order in (None, list(range(m))[::-1], list(np.random.default_rng(pf).permutation(m))):
        (wq, wb, _), (gq, gb, _, steps) = run(x, x["neg"], bias, pf, groups, order)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb), (pf, groups, order)
        assert np.array_equal(wq[0], x["Q0"][0]) and all(not np.array_equal(wq[r], x["Q0"][r]) for r in range(1, m))
        assert np.array_equal(wb, x["b0"]) != bias
        # a row costs its triples + 3 pf steps of fill and drain, + at most pf - 1 idle steps to ring slot 0
        rows_with_triples = sum(1 for k in LENGTHS if k)
        assert steps <= EPOCHS * sum(LENGTHS) + rows_with_triples * (4 * pf - 1)


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_draws_every_negative_on_its_own_users_row(pf, groups):
    x = inputs()
    for seen in (x["seen"], None):
        (wq, wb, wn), (gq, gb, gn, _) = run(x, draw, True, pf, groups, list(np.random.default_rng(3).permutation(len(LENGTHS))),
                                            seen=seen)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb) and np.array_equal(gn, wn)
    users_of = np.tile(x["users"], EPOCHS)
    (_, _, wn), _ = run(x, draw, True, pf, groups, seen=x["seen"])
    assert (wn[users_of == 3] == 23).all() and (wn[users_of == 4] == 0).all() and (users_of == 4).any()
    assert (wn[users_of != 4] >= 1).all()


def test_pipeline_on_a_slice_of_a_larger_csr_and_with_bad_ids():
    x = inputs(base=5)
    (wq, wb, _), (gq, gb, _, _) = run(x, x["neg"], True, 2, 2)
    assert np.array_equal(gq, wq) and np.array_equal(gb, wb)
    # an order entry out of range is passed over
    m = len(LENGTHS)
    order = [7, 99, 6, 5, -1, 4, 3, m, 10, 8, m + 5]
    _, (gq, gb, _, _) = run(x, x["neg"], True, 2, 2, order)
    kept = [r for r in order if 0 <= r < m]
    untouched = [r for r in range(m) if r not in kept]
    assert np.array_equal(gq[kept], wq[kept]) and np.array_equal(gb[kept], wb[kept])
    assert np.array_equal(gq[untouched], x["Q0"][untouched]) and np.array_equal(gb[untouched], x["b0"][untouched])
    # a user or a given negative out of range skips its triple, as a negative 0 does
    bad_neg, bad_users = x["neg"].copy(), x["users"].copy()
    bad_neg[5], bad_neg[40] = I, -5
    bad_users[5 + 8], bad_users[5 + 30] = -1, U
    zero = bad_neg.copy()
    zero[[5, 40]] = 0
    for e in range(EPOCHS):
        zero[e * sum(LENGTHS) + np.array([8, 30])] = 0
    want = restate(x["P"], x["Q"], x["bias"], x["indptr"], x["users"], zero, x["Q0"], x["b0"], EPOCHS, 0.05, 0.0)
    y = dict(x, users=bad_users)
    for neg in (bad_neg, draw):
        (wq, wb, wn), (gq, gb, gn, _) = run(y, neg, True, 4, 2, reg=0.0, seen=x["seen"] if neg is draw else None)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb)
        if neg is draw:
            assert np.array_equal(gn, wn)
        else:
            assert np.array_equal(gq, want[0]) and np.array_equal(gb, want[1])
