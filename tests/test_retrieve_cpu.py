"""Deep retrieval on a machine without a GPU: argument validation of `bpr_retrieve_rows` / `bpr_retrieve_workspace` /
`bpr_retrieve_slices` (nothing touches the device before the arguments are checked), the launch plan
(revisit-bpr_amd/csrc/bpr_retrieve_plan.h — through the library's test hook `bpr_test_retrieve_plan`, and alone in a
host program built under the host sanitizers), the numpy model of the selection (tests/retrieve_model.py) against a
brute-force sort, and the Python wrapper's refusals.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from retrieve_model import TI, brute_force, cap_of, retrieve_row

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
TU = 64  # users of a workgroup (bpr_topk_plan.h)
LDS_CU = 163_840
FIELDS = ("slices", "user_tiles", "item_tiles", "tile_users", "tile_items", "cap", "lds", "merge_lds", "ws_bytes",
          "units", "grid", "grid_max", "part_bytes", "buf_bytes")


def lib():
    from revisit_bpr import native

    return native.load()


def rows(P=1, Q=1, I=100, d=8, users=1, n=4, k=10, item_slices=0, ws=8, ws_bytes=1 << 40, items=1, scores=1):
    """bpr_retrieve_rows with fake non-NULL pointers where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0, go through here."""
    return lib().bpr_retrieve_rows(P, Q, None, I, d, users, n, None, None, k, item_slices, ws, ws_bytes, items, scores,
                                   None)


def workspace(n, I=20109, d=128, k=1000, item_slices=0):
    out = ctypes.c_int64(-1)
    assert lib().bpr_retrieve_workspace(n, I, d, k, item_slices, ctypes.byref(out)) == 0
    return out.value


def plan(n, I, d=128, k=1000, item_slices=0, cus=256):
    fn = lib().bpr_test_retrieve_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 3
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    bounds = (ctypes.c_int64 * 65)()
    assert fn((ctypes.c_int64 * 6)(n, I, d, k, item_slices, cus), out, bounds) == 0
    p = dict(zip(FIELDS, out))
    p["bounds"] = list(bounds[:p["slices"] + 1])
    return p


# ---- 1. arguments ------------------------------------------------------------------------------------------------
# (n = 4, I = 100, k = 10 needs one slice and one block of 64 x 256 candidates)
@pytest.mark.parametrize("kw, word", [
    (dict(P=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(users=None), b"NULL"), (dict(items=None), b"NULL"),
    (dict(scores=None), b"NULL"), (dict(k=0), b"k must be"), (dict(k=1025), b"1024"), (dict(d=0), b"d must be"),
    (dict(d=1025), b"1024"), (dict(I=0), b"I in"), (dict(n=-1), b"n must be"), (dict(item_slices=-1), b"item_slices"),
    (dict(item_slices=65), b"item_slices"), (dict(n=2 ** 31), b"2^31"),
    (dict(ws=None, ws_bytes=1 << 40), b"workspace"), (dict(ws=None, ws_bytes=0), b"workspace"),
    (dict(ws=8, ws_bytes=64 * 256 * 8 - 1), b"workspace"),
    (dict(item_slices=4, I=5000, ws=8, ws_bytes=4 * 4 * 10 * 8 + 4 * 64 * 256 * 8 - 1), b"workspace"),
    (dict(ws=4), b"aligned"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_users_is_ok_without_tables_or_workspace():
    assert rows(P=None, Q=None, users=None, items=None, scores=None, n=0, ws=None, ws_bytes=0) == 0
    assert rows(P=None, Q=None, users=None, items=None, scores=None, n=0, ws=None, ws_bytes=0, k=1025) == -1
    assert workspace(0) == 0 and workspace(0, item_slices=8) == 0


def test_the_workspace_is_always_needed():
    """even one slice keeps its candidates in device memory: one block of TU x cap pairs per persistent workgroup"""
    assert workspace(4, I=100, k=10, item_slices=1) == 64 * 256 * 8 > 0
    assert plan(4, 100, k=10)["ws_bytes"] == 64 * 256 * 8  # (100 items: one tile, one slice)
    assert workspace(1, k=1024, item_slices=1) == 64 * 2048 * 8


def test_workspace_and_slices_refuse_bad_shapes():
    out, out32 = ctypes.c_int64(), ctypes.c_int32()
    for args in ((4, 100, 8, 0, 0), (4, 100, 8, 1025, 0), (4, 100, 0, 10, 0), (4, 100, 1025, 10, 0), (4, 0, 8, 10, 0),
                 (-1, 100, 8, 10, 0), (4, 100, 8, 10, 65), (4, 100, 8, 10, -1), (2 ** 31, 100, 8, 10, 0)):
        assert lib().bpr_retrieve_workspace(*args, ctypes.byref(out)) == -1
        assert lib().bpr_last_error()
        assert lib().bpr_retrieve_slices(*args, ctypes.byref(out32)) == -1
    assert lib().bpr_retrieve_workspace(4, 100, 8, 10, 0, None) == -1
    assert lib().bpr_retrieve_slices(4, 100, 8, 10, 0, None) == -1
    assert lib().bpr_retrieve_workspace(4, 100, 8, 1024, 64, ctypes.byref(out)) == 0  # (k = 1024 is in range)


# ---- 2. the plan -------------------------------------------------------------------------------------------------
def test_cap_lds_and_slices_for_every_k():
    for k in range(1, 1025):
        p = plan(1000, 20109, k=k, item_slices=64)
        assert p["cap"] >= k + TI and p["cap"] >= 2 * k and p["cap"] == cap_of(k)
        assert 0 < p["lds"] <= LDS_CU
        assert p["slices"] * k <= 8192 and p["slices"] == min(64, 8192 // k)  # (158 item tiles: never the limit)
        assert 0 < p["merge_lds"] <= 64 * 1024 + 1024
        assert plan(1, 20109, k=k)["slices"] * k <= 8192
        assert (p["tile_users"], p["tile_items"]) == (TU, TI)
    assert plan(1, 20109, k=1024)["slices"] == 8 and plan(1, 20109, k=1024, item_slices=64)["slices"] == 8
    assert plan(1, 20109, k=128)["slices"] == 64
    assert plan(1, 20109, k=1024, item_slices=1)["merge_lds"] == 0


def test_a_larger_slice_count_is_reduced_and_reported():
    out = ctypes.c_int32(-1)
    for n, I, k, given in ((1, 20109, 1024, 0), (1, 20109, 1024, 64), (1, 20109, 1024, 3), (130, 5000, 1000, 64),
                           (130, 5000, 129, 64), (10_000, 200, 300, 7), (138_493, 20109, 512, 0), (1, 1, 5, 9)):
        assert lib().bpr_retrieve_slices(n, I, 128, k, given, ctypes.byref(out)) == 0
        p = plan(n, I, k=k, item_slices=given)
        assert out.value == p["slices"] <= min(64, 8192 // k, -(-I // TI))
        if given:
            assert out.value == min(given, 8192 // k, -(-I // TI))
        # asked for with that count, the workspace is the call's own need
        own = workspace(n, I=I, k=k, item_slices=out.value)
        assert own == p["ws_bytes"] <= workspace(n, I=I, k=k, item_slices=given)


@pytest.mark.parametrize("I", [1, 2, 127, 128, 129, 5000, 20109, 1_000_003])
def test_slices_cover_the_items_exactly_once(I):
    for k in (1, 128, 129, 1024):
        for item_slices in (0, 1, 2, 3, 7, 8, 64):
            for n in (1, 1000):
                p = plan(n, I, k=k, item_slices=item_slices)
                b = p["bounds"]
                assert b[0] == 0 and b[-1] == I and len(b) == p["slices"] + 1
                assert all(lo < hi for lo, hi in zip(b, b[1:])), b  # disjoint, in order, none empty
                assert all(x % TI == 0 for x in b[:-1])  # whole tiles


@pytest.mark.parametrize("k", [1, 128, 129, 256, 257, 1000, 1024])
@pytest.mark.parametrize("item_slices", [0, 1, 2, 8])
def test_persistent_grid_bounds_the_workspace(k, item_slices):
    """grid = min(units, grid_max), sized from the CUs; one block of TU x cap pairs each.  Past the grid's reach only
    the partial results of a given slice count grow with n; the library's choice has none there: constant."""
    ns = [0, 1, 2, 63, 64, 65, 130, 1000, 4096, 8191, 8192, 16_320, 16_321, 16_384, 20_000, 32_768, 32_769, 138_493,
          571_355, 2 ** 31 - 1]
    got = [workspace(n, k=k, item_slices=item_slices) for n in ns]
    assert all(a <= b for a, b in zip(got, got[1:])), list(zip(ns, got))  # never shrinks as n grows
    for n in ns:
        p = plan(n, 20109, k=k, item_slices=item_slices)
        assert p["units"] == p["user_tiles"] * p["slices"]
        assert p["grid"] == min(p["units"], p["grid_max"]) and p["grid_max"] in (256, 512)
        assert p["grid_max"] * p["lds"] <= 256 * LDS_CU  # what is resident at once fits the CUs' LDS
        assert p["buf_bytes"] == p["grid"] * TU * p["cap"] * 8
        assert p["part_bytes"] == (n * p["slices"] * k * 8 if p["slices"] > 1 else 0)
        assert p["ws_bytes"] == p["part_bytes"] + p["buf_bytes"] <= workspace(n, k=k, item_slices=item_slices)
    reach = plan(1, 20109, k=k)["grid_max"] * TU  # rows of grid_max user tiles
    far = [n for n in ns if n >= reach]
    assert len(far) >= 4
    if item_slices == 0:
        assert len({workspace(n, k=k) for n in far}) == 1  # constant in n
        # at most 255 user tiles ever share slices (slices x k <= 8192), and at most 512 blocks of TU x 2048 pairs
        assert workspace(far[0], k=k) <= 255 * TU * 8192 * 8 + 512 * TU * 2048 * 8
    else:
        bufs = {workspace(n, k=k, item_slices=item_slices) - plan(n, 20109, k=k, item_slices=item_slices)["part_bytes"]
                for n in far}
        assert len(bufs) == 1  # beyond the partial results: constant
    assert plan(2 ** 31 - 1, 20109, k=k, item_slices=item_slices)["user_tiles"] == 2 ** 25


def test_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """bpr_retrieve_plan.h is plain C++: built into a program of its own with -fsanitize=address,undefined, its sweep
    (tests/retrieve_plan_check.cpp: user counts past 2^31 / TU tiles and past 2^31 rows, every k) runs clean."""
    exe = tmp_path / "retrieve_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "retrieve_plan_check.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3. the selection model ----------------------------------------------------------------------------------------
def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("k, I", [(1, 700), (100, 3000), (128, 2000), (129, 3000), (300, 5000), (1000, 9000),
                                  (1024, 2047), (1024, 2048), (1024, 2049), (1024, 4225), (5, 2), (40, 30)])
def test_model_equals_brute_force_on_random_scores(k, I):
    rng = np.random.default_rng(k * 7 + I)
    scores = rng.standard_normal(I).astype(np.float32)
    scores[rng.integers(0, I, I // 50)] = np.nan  # never enter
    scores[rng.integers(0, I, I // 10)] = scores[rng.integers(0, I, I // 10)]  # ties
    seen = rng.choice(np.arange(1, I), size=(I - 1) // 5, replace=False) if I > 1 else ()
    want = brute_force(scores, k, seen)
    it, sc, row = retrieve_row(scores, k, seen)
    assert same((it, sc), want)
    assert row.high_water <= row.cap == cap_of(k)
    # the appends of each tile in another order: the same bits
    for seed in (1, 2):
        it2, sc2, _ = retrieve_row(scores, k, seen, rng=np.random.default_rng(seed))
        assert same((it2, sc2), want)
    # the tightest buffer the plan's rule allows gives the same result
    it3, sc3, tight = retrieve_row(scores, k, seen, cap=k + TI, rng=np.random.default_rng(3))
    assert same((it3, sc3), want) and tight.high_water <= k + TI


@pytest.mark.parametrize("k", [1, 128, 129, 1024])
def test_model_on_adversarial_scores(k):
    I = 3 * cap_of(k) + TI + 1
    ids = np.arange(I)
    # all equal: ids 1 .. k in order, and after the fill nothing beats tau
    it, sc, row = retrieve_row(np.zeros(I, np.float32), k)
    assert np.array_equal(it, np.arange(1, k + 1)) and (sc == 0).all()
    assert same((it, sc), brute_force(np.zeros(I, np.float32), k))
    # increasing with id: every item beats tau, compactions at their maximum — one per cap - k appended at least
    up = ids.astype(np.float32)
    it, sc, row_up = retrieve_row(up, k, rng=np.random.default_rng(0))
    assert np.array_equal(it, np.arange(I - 1, I - 1 - k, -1)) and same((it, sc), brute_force(up, k))
    assert row_up.compactions >= (I - 1 - row_up.cap) // row_up.cap >= 2 and row_up.high_water <= row_up.cap
    # decreasing with id: nothing beats tau after the first compaction
    down = (-ids).astype(np.float32)
    it, sc, row_down = retrieve_row(down, k, rng=np.random.default_rng(0))
    assert np.array_equal(it, np.arange(1, k + 1)) and same((it, sc), brute_force(down, k))
    assert row_down.compactions == 2 < row_up.compactions  # the one that sets tau, and the final one
    # a seen row that leaves 0 and 3 eligible items: padding
    for keep in (0, 3):
        seen = np.arange(1 + keep, I)
        it, sc, _ = retrieve_row(up, k, seen)
        assert same((it, sc), brute_force(up, k, seen))
        assert (it >= 0).sum() == min(keep, k) and np.isneginf(sc[min(keep, k):]).all()


def test_model_over_slices_merges_to_the_whole():
    """what the merge relies on: the k best of the whole are among the k best of the slices"""
    rng = np.random.default_rng(9)
    I, k = 5000, 257
    scores = rng.integers(-50, 50, I).astype(np.float32)
    want = brute_force(scores, k)
    parts = [retrieve_row(scores, k, lo=lo, hi=hi)[:2] for lo, hi in ((0, 1664), (1664, 3328), (3328, I))]
    ids = np.concatenate([p[0][p[0] >= 0] for p in parts])
    top = ids[np.lexsort((ids, -scores[ids].astype(np.float64)))][:k]
    assert np.array_equal(top, want[0])


# ---- 4. the wrapper ----------------------------------------------------------------------------------------------
def test_retrieve_refuses_cpu_tensors_and_bad_arguments():
    torch = pytest.importorskip("torch")
    from revisit_bpr import retrieve as mod
    from revisit_bpr.retrieve import RETRIEVE_MAX, retrieve

    P, Q, users = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        retrieve(P, Q, None, users, 3)
    with pytest.raises(RuntimeError):
        retrieve(P, Q, None, users, 1000)
    with pytest.raises(ValueError, match="1024"):
        retrieve(P, Q, None, users, 1025)
    with pytest.raises(ValueError):
        retrieve(P, Q, None, users, 0)
    assert RETRIEVE_MAX == 1024
    assert mod.slices(1, 20109, 128, 1024, 64) == 8 and mod.slices(138_493, 20109, 128, 1024) == 1
    assert mod.workspace_bytes(1, 20109, 128, 1024, 1) == 64 * 2048 * 8
    from revisit_bpr import native

    with pytest.raises(native.BprError, match="1024"):
        mod.workspace_bytes(1, 100, 8, 1025)
    from revisit_bpr.engine import Engine
    from revisit_bpr.models import BPR

    assert callable(Engine.retrieve) and callable(BPR.retrieve)
