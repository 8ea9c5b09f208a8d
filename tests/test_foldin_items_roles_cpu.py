"""Item fold-in in both roles (`bpr_fold_in_item_rows_roles`, `fold_in_items(neg_role=...)`) on a machine without a
GPU: the step schedule of the definition, the control-flow model of the kernel's ring against the definition
(tests/foldin_items_roles_model.py), the entry point's refusals (nothing touches the device before the arguments are
checked) and the Python wrapper's."""
import numpy as np
import pytest

from foldin_items_roles_model import ATTEMPTS, pipeline, restate, role_draw, role_words, schedule

INVALID, UNSUPPORTED = -1, -3
GIVEN, UNIFORM = 0, 1


# ---- the schedule ----------------------------------------------------------------------------------------------------
def test_schedule_places_exactly_R_negative_role_steps_in_order():
    for L in range(71):
        for R in range(71):
            steps = schedule(L, R)
            assert len(steps) == L + R
            assert [at for role, at in steps if role] == list(range(R)), (L, R)  # rho runs 0, 1, 2, ...
            assert [at for role, at in steps if not role] == list(range(L)), (L, R)  # and so does k
    assert all(role for role, _ in schedule(0, 5)) and not any(role for role, _ in schedule(5, 0))
    # evenly spread: between two negative-role steps lie floor or ceil of L / R positive-role steps
    where = [s for s, (role, _) in enumerate(schedule(64, 3)) if role]
    assert all(b - a - 1 in (21, 22) for a, b in zip(where, where[1:]))


def test_schedule_is_the_kernels_accumulator():
    """The kernel walks acc = s R mod (L + R) instead of dividing: step s is a negative-role step iff acc + R >= L + R."""
    for L, R in [(0, 1), (1, 1), (7, 3), (3, 7), (70, 1), (1, 70), (64, 40), (2 ** 20 + 3, 977)]:
        n, acc, got = L + R, 0, []
        for s in range(min(n, 5000)):
            role = acc + R >= n
            got.append(role)
            acc += R - (n if role else 0)
            assert acc == (s + 1) * R % n
        assert got == [(s + 1) * R // n > s * R // n for s in range(len(got))]


def test_philox_is_the_published_one():
    """Known-answer vectors of Philox4x32-10 (Random123's kat_vectors)."""
    from foldin_items_roles_model import philox4x32_10

    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert len(role_words(5, 2 ** 40 + 3)) == ATTEMPTS and role_words(5, 1) != role_words(5, 2) != role_words(6, 2)


# ---- the control-flow model ------------------------------------------------------------------------------------------
U, I, EPOCHS = 40, 50, 3
# A row drains through 3 pf further steps (3, 6, 12 at pf 1, 2, 4): with R = 0 the rows of 1, 2 and 4 users are exactly a
# drain long, with R = 1 the rows of 0, 1 and 3 users, with R = 3 the row of 1 user (pf 4); the others are shorter or
# longer.  The row of 40 users holds every user: none of its negative-role steps finds an interaction.
LENGTHS = [0, 1, 2, 3, 4, 6, 9, 12, 17, 33, 40]
SEEN_LENGTHS = [0, 1, 17, 48, 49] + [5] * (U - 5)  # user 3 has seen all but item 23, user 4 every item
T = 300


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
    train = (rng.integers(0, U, T).astype(np.int32), rng.integers(1, I, T).astype(np.int32))
    train[0][[3, 50]], train[1][[90, 200]] = (-1, U), (0, I)  # entries out of range: never accepted
    P = rng.normal(0, 0.5, (U, d))
    Q = rng.normal(0, 0.5, (I, d))
    Q[0] = 0
    m = len(LENGTHS)
    return dict(P=P, Q=Q, bias=rng.normal(0, 0.5, I), indptr=indptr, users=users, neg=neg, seen=seen, train=train,
                Q0=rng.normal(0, 0.1, (m, d)), b0=rng.normal(0, 0.1, m))


def draw(u, seen_row, t):
    """A stand-in for the device sampler: a pure function of (the user's seen row, the counter)."""
    unseen = np.setdiff1d(np.arange(1, I), seen_row)
    return int(unseen[(t * 2654435761 + 12345) % len(unseen)]) if len(unseen) else 0


def run(x, neg, bias, R, pf, groups, order=None, seen=None, reg=0.05, seed=9, offset=2 ** 33 + 5):
    b = x["bias"] if bias else None
    args = (x["P"], x["Q"], b, x["indptr"], x["users"], neg, x["Q0"], x["b0"], EPOCHS, 0.05, reg, R, x["train"], seed,
            offset)
    return restate(*args, seen=seen), pipeline(*args, pf, groups, order, seen=seen)


@pytest.mark.parametrize("R", [0, 1, 3, 40])
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_applies_the_definition_bit_for_bit(pf, groups, R):
    x = inputs()
    m = len(LENGTHS)
    orders = (None, list(range(m))[::-1], list(np.random.default_rng(pf).permutation(m)))
    for k, order in enumerate(orders):
        bias = (k + groups) % 2 == 0
        (wq, wb, _, wr), (gq, gb, _, gr, steps) = run(x, x["neg"], bias, R, pf, groups, order)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb) and np.array_equal(gr, wr), (pf, groups, order)
        assert np.array_equal(wq[0], x["Q0"][0]) == (R == 0)  # the row without an audience learns from its second role
        assert all(not np.array_equal(wq[r], x["Q0"][r]) for r in range(1, m))
        assert np.array_equal(wb, x["b0"]) != bias
        assert (wr >= -1).all() and wr.shape == (EPOCHS * m * R,)
        # a row costs its steps + 3 pf steps of fill and drain, + at most pf - 1 idle steps to ring slot 0
        rows_with_steps = sum(1 for k in LENGTHS if k + R)
        assert steps <= EPOCHS * (sum(LENGTHS) + m * R) + rows_with_steps * (4 * pf - 1)
        if R:
            per_row = wr.reshape(EPOCHS, m, R)
            assert (per_row[:, m - 1] == -1).all()  # everybody is in the last row's audience
            assert (per_row[:, :m - 2] >= 0).all()  # audiences of at most 17 of 40 users: 16 attempts suffice here
            for r in range(m):
                aud = set(x["users"][x["indptr"][r]:x["indptr"][r + 1]].tolist())
                taus = per_row[:, r][per_row[:, r] >= 0]
                assert not aud & set(x["train"][0][taus].tolist())
                assert not set(taus.tolist()) & {3, 50, 90, 200}


@pytest.mark.parametrize("R", [0, 3])
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("pf", [1, 2, 4])
def test_pipeline_with_sampled_negatives_and_the_same_positive_role_draws_at_every_R(pf, groups, R):
    x = inputs()
    order = list(np.random.default_rng(3).permutation(len(LENGTHS)))
    for seen in (x["seen"], None):
        (wq, wb, wn, wr), (gq, gb, gn, gr, _) = run(x, draw, True, R, pf, groups, order, seen=seen)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb) and np.array_equal(gn, wn) and np.array_equal(gr, wr)
        (_, _, n0, _), _ = run(x, draw, True, 0, pf, groups, order, seen=seen)
        assert np.array_equal(wn, n0)  # the positive-role draws do not depend on R


def test_R_0_is_the_single_role_definition():
    import foldin_items_model as old

    x = inputs()
    for neg, seen in ((x["neg"], None), (draw, x["seen"])):
        (wq, wb, wn, _), _ = run(x, neg, True, 0, 2, 2, seen=seen)
        lr = float(np.float32(0.05))  # (this model takes lr and reg_item as the fp32 values the kernel is given)
        oq, ob, on = old.restate(x["P"], x["Q"], x["bias"], x["indptr"], x["users"], neg, x["Q0"], x["b0"], EPOCHS, lr, lr,
                                 seen=seen)
        assert np.array_equal(wq, oq) and np.array_equal(wb, ob)
        assert np.array_equal(wn, on)


def test_pipeline_on_a_slice_of_a_larger_csr_with_holes_in_the_order_and_bad_ids():
    x = inputs(base=5)
    (wq, wb, _, wr), (gq, gb, _, gr, _) = run(x, x["neg"], True, 3, 2, 2)
    assert np.array_equal(gq, wq) and np.array_equal(gb, wb) and np.array_equal(gr, wr)
    m = len(LENGTHS)
    order = [7, 99, 6, 5, -1, 4, 3, m, 10, 8, m + 5]  # an order entry out of range is passed over
    _, (gq, gb, _, gr, _) = run(x, x["neg"], True, 3, 2, 2, order)
    kept = [r for r in order if 0 <= r < m]
    untouched = [r for r in range(m) if r not in kept]
    assert np.array_equal(gq[kept], wq[kept]) and np.array_equal(gb[kept], wb[kept])
    assert np.array_equal(gq[untouched], x["Q0"][untouched]) and np.array_equal(gb[untouched], x["b0"][untouched])
    gr, wr = gr.reshape(EPOCHS, m, 3), wr.reshape(EPOCHS, m, 3)
    assert np.array_equal(gr[:, kept], wr[:, kept]) and (gr[:, untouched] == -7).all()  # their entries are not written
    bad_users = x["users"].copy()  # (ids out of range that keep their rows sorted: the audience search relies on it)
    first_of_6, last_of_9 = int(x["indptr"][6]), int(x["indptr"][10]) - 1
    bad_users[first_of_6], bad_users[last_of_9] = -1, U
    y = dict(x, users=bad_users)
    for neg in (x["neg"], draw):
        (wq, wb, wn, wr), (gq, gb, gn, gr, _) = run(y, neg, True, 3, 4, 2, reg=0.0, seen=x["seen"] if neg is draw else None)
        assert np.array_equal(gq, wq) and np.array_equal(gb, wb) and np.array_equal(gr, wr)
        assert neg is not draw or np.array_equal(gn, wn)


def test_a_draw_depends_on_seed_counter_and_audience_only():
    x = inputs()
    aud = x["users"][x["indptr"][8]:x["indptr"][9]]
    a = [role_draw(x["train"], U, I, aud, 9, c) for c in range(100, 140)]
    assert a == [role_draw(x["train"], U, I, aud, 9, c) for c in range(100, 140)]
    assert a != [role_draw(x["train"], U, I, aud, 10, c) for c in range(100, 140)]
    assert len(set(a)) > 20 and min(a) >= 0
    assert role_draw(x["train"], U, I, np.arange(U), 9, 100) == -1


# ---- the entry point's refusals --------------------------------------------------------------------------------------
def lib():
    from revisit_bpr import native

    return native.load()


def rows(m=4, epochs=3, train_users=1, train_items=1, T=10, R=2, role_out=None, d=8, sampler=UNIFORM, P=1, indptr=1):
    """bpr_fold_in_item_rows_roles with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be
    refused before the device is touched, or m = 0, go through here."""
    return lib().bpr_fold_in_item_rows_roles(P, 40, 1, None, 100, d, None, None, indptr, 1, m, None, epochs, 0.05, 0.0,
                                             sampler, None, None, 0, 0, train_users, train_items, T, R, role_out, 1,
                                             None, None)


@pytest.mark.parametrize("kw, status, word", [
    (dict(R=-1), INVALID, b"neg_role"), (dict(train_users=None), INVALID, b"train_users"),
    (dict(train_items=None), INVALID, b"train_items"), (dict(T=0), INVALID, b"T of at least 1"),
    (dict(T=-5), INVALID, b"T of at least 1"), (dict(T=2 ** 31), UNSUPPORTED, b"T must be below"),
    (dict(m=2 ** 20, epochs=2 ** 5, R=2 ** 6), UNSUPPORTED, b"epochs * m * neg_role"),
    (dict(m=1, epochs=1, R=2 ** 31 - 1, P=None), INVALID, b"NULL"),  # (the bound itself is allowed)
    (dict(d=0), INVALID, b"d must be"), (dict(d=1025), UNSUPPORTED, b"1024"), (dict(epochs=0), INVALID, b"epochs"),
    (dict(sampler=2), UNSUPPORTED, b"adaptive"), (dict(sampler=GIVEN), INVALID, b"neg_in"),
    (dict(R=0, train_users=None, train_items=None, T=0, indptr=None), INVALID, b"NULL"),  # (R = 0 accepts no arrays)
])
def test_bad_arguments_are_refused_without_a_device(kw, status, word):
    assert rows(**kw) == status
    err = lib().bpr_last_error()
    assert b"bpr_fold_in_item_rows_roles" in err and word in err, err


def test_no_rows_is_ok_without_tables():
    assert rows(m=0, P=None, indptr=None) == 0
    assert rows(m=0, P=None, indptr=None, R=0, train_users=None, train_items=None, T=0) == 0
    assert rows(m=0, R=-1) == INVALID  # (still validated)
    assert rows(m=0, train_users=None) == INVALID


# ---- the wrapper's refusals ------------------------------------------------------------------------------------------
def wrapper_inputs():
    import torch

    return dict(P=torch.zeros(5, 8), Q=torch.zeros(6, 8), item_bias=None,
                indptr=torch.tensor([0, 2, 3], dtype=torch.int64), users=torch.tensor([1, 4, 2], dtype=torch.int32),
                epochs=2, lr=0.05, neg_role=2, train_users=torch.tensor([1, 2, 3], dtype=torch.int32),
                train_items=torch.tensor([1, 2, 3], dtype=torch.int32))


def call(args):
    from revisit_bpr.foldin_items import fold_in_items

    args = dict(args)
    return fold_in_items(args.pop("P"), args.pop("Q"), args.pop("item_bias"), args.pop("indptr"), args.pop("users"),
                         **args)


def test_wrapper_refuses_bad_role_arguments_without_a_device():
    torch = pytest.importorskip("torch")
    ok = wrapper_inputs()
    i32 = torch.int32
    for bad in (dict(neg_role=-1), dict(neg_role="often"), dict(neg_role=1.5), dict(neg_role=True),
                dict(train_users=None), dict(train_items=None), dict(train_users=None, train_items=None),
                dict(neg_role="auto", train_users=None), dict(neg_role="auto", train_users=None, train_items=None),
                dict(train_users=ok["train_users"].long()), dict(train_items=ok["train_items"].long()),
                dict(train_items=torch.ones(4, dtype=i32)),  # not the length of train_users
                dict(train_users=torch.ones(0, dtype=i32), train_items=torch.ones(0, dtype=i32)),
                dict(neg_role=2 ** 29)):  # epochs * m * R
        with pytest.raises(ValueError):
            call(dict(ok, **bad))
    for fine in (ok, dict(ok, neg_role="auto"), dict(ok, neg_role=0, train_users=None, train_items=None)):
        with pytest.raises(RuntimeError, match="ROCm"):  # the arguments pass; there is no CPU path
            call(fine)


def test_auto_is_the_expected_count_of_joint_uniform_training():
    torch = pytest.importorskip("torch")
    from revisit_bpr.foldin_items import _roles

    t = torch.ones(1000, dtype=torch.int32)
    assert _roles("auto", t, t, 101)[0] == 10 and _roles("auto", t, t, 5001)[0] == 1 and _roles("auto", t, t, 41)[0] == 25
    assert _roles(7, t, t, 101)[0] == 7 and _roles(0, None, None, 101) == (0, None, None)
