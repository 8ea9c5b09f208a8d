"""Fold-in (`bpr_fold_in_rows`, revisit_bpr/foldin.py) on a machine without a GPU: the launch plan
(revisit-bpr_amd/csrc/bpr_foldin_plan.h, through the library's test hook `bpr_test_foldin_plan`), the argument
validation of the entry point (nothing touches the device before the arguments are checked) and the Python
wrapper's refusals.  Integer arithmetic only: no GPU."""
import ctypes

import pytest

FIELDS = ("G", "E", "block", "groups_per_block", "pf", "groups", "grid", "resident")
INVALID, UNSUPPORTED = -1, -3
GIVEN, UNIFORM, ADAPTIVE = 0, 1, 2


def lib():
    from revisit_bpr import native

    return native.load()


def plan(n, d, cus=256):
    fn = lib().bpr_test_foldin_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 3)(n, d, cus), out) == 0
    return dict(zip(FIELDS, out))


def rows(Q=1, bias=None, I=100, d=8, indptr=1, items=1, n=4, order=None, epochs=3, lr=0.05, alpha=0.0,
         sampler=UNIFORM, neg_in=None, neg_out=None, P=1):
    """bpr_fold_in_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0, go through here."""
    return lib().bpr_fold_in_rows(Q, bias, I, d, indptr, items, n, order, epochs, lr, alpha, sampler, neg_in, neg_out,
                                  0, 0, P, None)


@pytest.mark.parametrize("d, G, E", [(1, 32, 1), (32, 32, 1), (33, 32, 2), (64, 32, 2), (65, 32, 4), (128, 32, 4),
                                     (129, 64, 4), (256, 64, 4), (257, 64, 8), (512, 64, 8), (513, 64, 16),
                                     (1024, 64, 16)])
def test_plan_group_width_by_d(d, G, E):
    p = plan(1000, d)
    assert (p["G"], p["E"]) == (G, E) and G * E >= d
    assert p["block"] == 256 and p["groups_per_block"] == 256 // G
    assert p["pf"] >= 1


@pytest.mark.parametrize("d", [8, 128, 256])
def test_plan_grid_never_exceeds_the_rows_and_is_capped_by_the_cus(d):
    gpb = plan(1, d)["groups_per_block"]
    for n in (0, 1, gpb - 1, gpb, gpb + 1, 1000, 10_000, 138_493, 2 ** 31 - 1):
        for cus in (1, 8, 256, 304):
            p = plan(n, d, cus)
            cap = cus * p["resident"] * gpb
            assert p["groups"] == min(n, cap)  # a group per row until the chip is full
            assert p["grid"] == -(-p["groups"] // gpb) <= cus * p["resident"]
            assert (p["grid"] - 1) * gpb < max(p["groups"], 1)  # no workgroup without a group


def test_plan_small_lists():
    assert plan(0, 128)["grid"] == 0 and plan(0, 128)["groups"] == 0
    assert (plan(1, 128)["grid"], plan(1, 128)["groups"]) == (1, 1)
    assert [plan(n, 128)["grid"] for n in (7, 8, 9)] == [1, 1, 2]  # 8 groups of 32 lanes in a workgroup
    assert [plan(n, 256)["grid"] for n in (3, 4, 5)] == [1, 1, 2]  # 4 groups of 64
    assert plan(10 ** 6, 128, cus=256)["grid"] == 256 * plan(1, 128)["resident"]
    out = (ctypes.c_int64 * len(FIELDS))()
    fn = lib().bpr_test_foldin_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    assert fn((ctypes.c_int64 * 3)(4, 0, 0), out) == INVALID
    assert fn((ctypes.c_int64 * 3)(4, 1025, 0), out) == UNSUPPORTED
    assert fn((ctypes.c_int64 * 3)(-1, 8, 0), out) == INVALID


@pytest.mark.parametrize("kw, status, word", [
    (dict(Q=None), INVALID, b"NULL"), (dict(indptr=None), INVALID, b"NULL"), (dict(items=None), INVALID, b"NULL"),
    (dict(P=None), INVALID, b"NULL"), (dict(epochs=0), INVALID, b"epochs"), (dict(epochs=-3), INVALID, b"epochs"),
    (dict(d=0), INVALID, b"d must be"), (dict(d=1025), UNSUPPORTED, b"1024"),
    (dict(sampler=GIVEN, neg_in=None), INVALID, b"neg_in"), (dict(sampler=7), INVALID, b"sampler"),
    (dict(sampler=-1), INVALID, b"sampler"), (dict(sampler=ADAPTIVE), UNSUPPORTED, b"adaptive"),
    (dict(n=-1), INVALID, b"n must be"), (dict(n=2 ** 31), INVALID, b"2^31"), (dict(I=0), INVALID, b"I must be"),
    (dict(I=2 ** 21, d=1024), UNSUPPORTED, b"I * d"), (dict(lr=float("nan")), INVALID, b"NaN"),
])
def test_bad_arguments_are_refused_without_a_device(kw, status, word):
    assert rows(**kw) == status
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_rows_is_ok_without_tables():
    assert rows(Q=None, indptr=None, items=None, P=None, n=0) == 0
    assert rows(Q=None, indptr=None, items=None, P=None, n=0, sampler=GIVEN) == 0
    assert rows(Q=None, indptr=None, items=None, P=None, n=0, epochs=0) == INVALID  # (still validated)
    assert rows(Q=None, indptr=None, items=None, P=None, n=0, d=1025) == UNSUPPORTED


def test_wrapper_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    import revisit_bpr
    from revisit_bpr.foldin import fold_in

    assert revisit_bpr.fold_in is fold_in
    Q = torch.zeros(6, 8)
    indptr = torch.tensor([0, 2, 3], dtype=torch.int64)
    items = torch.tensor([1, 4, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, None, indptr, items, epochs=2, lr=0.05)
    with pytest.raises(RuntimeError, match="ROCm"):
        fold_in(Q, torch.zeros(6), indptr, items, epochs=2, lr=0.05, neg=torch.ones(6, dtype=torch.int32))


def test_wrapper_refuses_wrong_dtypes_and_lengths():
    torch = pytest.importorskip("torch")
    from revisit_bpr.foldin import fold_in

    Q = torch.zeros(6, 8)
    indptr = torch.tensor([0, 2, 3], dtype=torch.int64)
    items = torch.tensor([1, 4, 2], dtype=torch.int32)
    ok = dict(epochs=2, lr=0.05)
    for bad in (dict(Q=Q.double()), dict(indptr=indptr.int()), dict(items=items.long()), dict(item_bias=torch.zeros(5)),
                dict(item_bias=torch.zeros(6, dtype=torch.float64)), dict(Q=torch.zeros(6)),
                dict(indptr=torch.tensor([0, 2, 4], dtype=torch.int64)),  # rows past the end of `items`
                dict(indptr=torch.tensor([2, 1], dtype=torch.int64)), dict(indptr=torch.zeros(0, dtype=torch.int64)),
                dict(neg=torch.ones(5, dtype=torch.int32)), dict(neg=torch.ones(7, dtype=torch.int32)),
                dict(neg=torch.ones(6, dtype=torch.int64)), dict(init=torch.zeros(3, 8)), dict(init=torch.zeros(2, 4)),
                dict(init=torch.zeros(2, 8, dtype=torch.float64)), dict(epochs=0)):
        args = dict(Q=Q, item_bias=None, indptr=indptr, items=items, **ok)
        args.update(bad)
        with pytest.raises(ValueError):
            fold_in(args.pop("Q"), args.pop("item_bias"), args.pop("indptr"), args.pop("items"), **args)


def test_balance_order_is_a_permutation_longest_first():
    torch = pytest.importorskip("torch")
    from revisit_bpr.foldin import balance_order

    g = torch.Generator().manual_seed(5)
    for n in (0, 1, 2, 17, 1000):
        lengths = torch.randint(0, 50, (n,), generator=g)
        order = balance_order(lengths)
        assert order.dtype == torch.int32 and order.shape == (n,)
        assert sorted(order.tolist()) == list(range(n))
        got = lengths[order.long()]
        assert bool((got[:-1] >= got[1:]).all())
    # ties keep list order (a stable sort): the order is a pure function of the lengths
    assert balance_order(torch.tensor([3, 9, 3, 9, 0])).tolist() == [1, 3, 0, 2, 4]
