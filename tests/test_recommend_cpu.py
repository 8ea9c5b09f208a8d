"""The fused top-K entry points on a machine without a GPU: argument validation of `bpr_topk_rows` /
`bpr_topk_workspace` (nothing touches the device before the arguments are checked), the launch plan
(revisit-bpr_amd/csrc/bpr_topk_plan.h, through the library's test hook `bpr_test_topk_plan`) and the Python wrapper's
refusals.  Integer arithmetic only: no GPU."""
import ctypes

import pytest

TU, TI = 64, 128  # users of a workgroup, items of a tile (bpr_topk_plan.h)
FIELDS = ("slices", "user_tiles", "item_tiles", "tile_users", "tile_items", "cap", "lds", "merge_lds", "ws_bytes")


def lib():
    from revisit_bpr import native

    return native.load()


def rows(P=1, Q=1, I=100, d=8, users=1, n=4, k=10, item_slices=0, ws=None, ws_bytes=0, items=1, scores=1):
    """bpr_topk_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0, go through here."""
    return lib().bpr_topk_rows(P, Q, None, I, d, users, n, None, None, k, item_slices, ws, ws_bytes, items, scores, None)


def workspace(n, I=20109, d=128, k=100, item_slices=0):
    out = ctypes.c_int64(-1)
    assert lib().bpr_topk_workspace(n, I, d, k, item_slices, ctypes.byref(out)) == 0
    return out.value


def plan(n, I, d=128, k=100, item_slices=0, cus=256):
    fn = lib().bpr_test_topk_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 3
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    bounds = (ctypes.c_int64 * 65)()
    assert fn((ctypes.c_int64 * 6)(n, I, d, k, item_slices, cus), out, bounds) == 0
    p = dict(zip(FIELDS, out))
    p["bounds"] = list(bounds[:p["slices"] + 1])
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(P=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(users=None), b"NULL"), (dict(items=None), b"NULL"),
    (dict(scores=None), b"NULL"), (dict(k=0), b"k must be"), (dict(k=129), b"128"), (dict(d=0), b"d must be"),
    (dict(d=1025), b"1024"), (dict(I=0), b"I in"), (dict(n=-1), b"n must be"), (dict(item_slices=-1), b"item_slices"),
    (dict(item_slices=65), b"item_slices"),
    (dict(item_slices=4, I=5000, ws=None, ws_bytes=0), b"workspace"),
    (dict(item_slices=4, I=5000, ws=1, ws_bytes=4 * 4 * 10 * 8 - 1), b"workspace"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_users_is_ok_without_tables():
    assert rows(P=None, Q=None, users=None, items=None, scores=None, n=0) == 0
    assert rows(P=None, Q=None, users=None, items=None, scores=None, n=0, k=129) == -1  # (still validated)


def test_workspace_refuses_bad_shapes():
    out = ctypes.c_int64()
    for args in ((4, 100, 8, 0, 0), (4, 100, 8, 129, 0), (4, 100, 0, 10, 0), (4, 100, 1025, 10, 0), (4, 0, 8, 10, 0),
                 (-1, 100, 8, 10, 0), (4, 100, 8, 10, 65)):
        assert lib().bpr_topk_workspace(*args, ctypes.byref(out)) == -1
        assert lib().bpr_last_error()
    assert lib().bpr_topk_workspace(4, 100, 8, 10, 0, None) == -1


@pytest.mark.parametrize("item_slices", [0, 1, 2, 7, 64])
@pytest.mark.parametrize("k", [1, 100, 128])
def test_workspace_is_monotone_in_n(item_slices, k):
    ns = [0, 1, 2, 63, 64, 65, 255, 256, 1000, 4096, 8191, 8192, 10_000, 16_000, 16_320, 16_321, 16_384, 20_000,
          138_493, 571_355]
    got = [workspace(n, k=k, item_slices=item_slices) for n in ns]
    assert all(b >= 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), list(zip(ns, got))


def test_workspace_bounds():
    """One slice: the kernel writes the result itself, no partial buffers.  s slices: exactly the partial results,
    s * n * k * 8 bytes — the constant on top is 0.  The library's choice: never more than its cap of 64 slices
    over fewer than 256 user tiles of 64."""
    for n in (0, 1, 64, 1000, 138_493):
        assert workspace(n, item_slices=1) == 0
        for s in (2, 7, 64):
            assert workspace(n, item_slices=s) == s * n * 100 * 8  # (20,109 items: 158 tiles >= 64 slices)
        assert workspace(n) <= 64 * 255 * 64 * 100 * 8
    assert workspace(1000, I=300, item_slices=7) == 3 * 1000 * 100 * 8  # 3 item tiles: 3 slices at most
    # what a call needs is the plan's own figure; the choice's answer covers it for every n
    for n in (1, 100, 5000, 16_000, 16_384, 138_493):
        assert plan(n, 20109)["ws_bytes"] <= workspace(n)


def test_slices_entry_point_is_the_plans_choice():
    """`bpr_topk_slices`: the count a call runs with; asked for with that count, the workspace is the call's own need
    (0 for one slice) instead of the never-shrinking bound of item_slices = 0."""
    out = ctypes.c_int32(-1)
    for n, I, given in ((1, 20109, 0), (256, 20109, 0), (10_000, 20109, 0), (138_493, 20109, 0), (10_000, 200, 7),
                        (20_000, 20109, 0)):
        assert lib().bpr_topk_slices(n, I, 128, 100, given, ctypes.byref(out)) == 0
        p = plan(n, I, item_slices=given)
        assert out.value == p["slices"]
        assert workspace(n, I=I, item_slices=out.value) == p["ws_bytes"] <= workspace(n, I=I, item_slices=given)
    assert workspace(20_000, item_slices=1) == 0 < workspace(20_000)
    assert lib().bpr_topk_slices(4, 100, 8, 129, 0, ctypes.byref(out)) == -1
    assert lib().bpr_topk_slices(4, 100, 8, 10, 0, None) == -1


def test_n_past_the_grid_limit_is_refused():
    assert rows(n=2 ** 31) == -1 and b"2^31" in lib().bpr_last_error()
    out = ctypes.c_int64()
    assert lib().bpr_topk_workspace(2 ** 31, 100, 8, 10, 0, ctypes.byref(out)) == -1


def test_plan_slices_by_the_user_tiles():
    assert plan(256 * TU, 20109)["slices"] == 1  # 256 user tiles: one per CU
    assert plan(256 * TU - TU + 1, 20109)["slices"] == 1
    assert plan(138_493, 20109)["slices"] == 1
    assert plan(255 * TU, 20109)["slices"] == 2
    p = plan(1, 20109)
    assert p["slices"] == 64 and p["user_tiles"] == 1 and p["item_tiles"] == 158  # capped at 64
    assert plan(1, 1000)["slices"] == 8  # ... and at the item tiles
    assert plan(1, 1)["slices"] == 1
    assert plan(256, 20109)["slices"] == 64  # 4 user tiles x 64 slices = 256 workgroups
    assert plan(10_000, 20109)["slices"] == 2  # 157 user tiles
    assert plan(10_000, 20109, item_slices=7)["slices"] == 7
    assert plan(10_000, 200, item_slices=7)["slices"] == 2  # no empty slices
    assert plan(0, 20109)["user_tiles"] == 0
    assert (p["tile_users"], p["tile_items"]) == (TU, TI)


@pytest.mark.parametrize("I", [1, 2, 127, 128, 129, 257, 5000, 20109, 41140, 1_000_003])
def test_slices_cover_the_items_exactly_once(I):
    for item_slices in (0, 1, 2, 3, 7, 64):
        for n in (1, 1000):
            p = plan(n, I, item_slices=item_slices)
            b = p["bounds"]
            assert b[0] == 0 and b[-1] == I and len(b) == p["slices"] + 1
            assert all(lo < hi for lo, hi in zip(b, b[1:])), b  # disjoint, in order, none empty
            assert all(x % TI == 0 for x in b[:-1])  # whole tiles


@pytest.mark.parametrize("d", [1, 32, 128, 256, 1024])
def test_lds_fits_a_cu(d):
    for k in (1, 10, 100, 128):
        p = plan(1000, 20109, d=d, k=k, item_slices=64)
        assert 0 < p["lds"] <= 160 * 1024
        assert p["cap"] == k + TI  # the k best of the last compaction + the most one tile can add
        assert 0 < p["merge_lds"] <= 64 * 1024 + 1024


def test_recommend_refuses_cpu_tensors_and_large_k():
    torch = pytest.importorskip("torch")
    from revisit_bpr.recommend import TOPK_MAX, recommend

    P, Q, users = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        recommend(P, Q, None, users, 3)
    with pytest.raises(ValueError, match="128"):
        recommend(P, Q, None, users, 129)
    with pytest.raises(ValueError):
        recommend(P, Q, None, users, 0)
    assert TOPK_MAX == 128
    from revisit_bpr.evaluation import evaluate_fused

    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="evaluate_topk"):
        evaluate_fused(torch.zeros(4, 8), torch.zeros(200, 8), None, users, z, z, z, z, ks=(5, 129))
