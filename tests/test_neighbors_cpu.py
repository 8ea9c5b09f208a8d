"""The fused neighbour entry points on a machine without a GPU: argument validation of `bpr_neighbors_rows` /
`bpr_neighbors_workspace` / `bpr_neighbors_slices` (nothing touches the device before the arguments are checked), the
launch plan (revisit-bpr_amd/csrc/bpr_neighbors_plan.h, through the library's test hook `bpr_test_neighbors_plan`) and
the Python wrapper's refusals.  Integer arithmetic only: no GPU."""
import ctypes
import re
from pathlib import Path

import pytest

TU, TI, KC, LD = 64, 128, 32, 36  # queries of a workgroup, table rows of a tile, staged features, floats of a staged row
LDS_CU = 163_840                  # bytes of LDS of a gfx950 CU
DOT, COSINE = 0, 1
FIELDS = ("slices", "query_tiles", "table_tiles", "tile_queries", "tile_rows", "cap", "lds", "lds_limit", "merge_lds",
          "partial_bytes", "norm_bytes", "ws_bytes")


def lib():
    from revisit_bpr import native

    return native.load()


def rows(X=1, T=1, N=100, d=8, rows=1, n=4, exclude=None, first=0, metric=DOT, k=10, item_slices=0, ws=None,
         ws_bytes=0, ids=1, scores=1):
    """bpr_neighbors_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0, go through here."""
    return lib().bpr_neighbors_rows(X, T, N, d, rows, n, exclude, first, metric, k, item_slices, ws, ws_bytes, ids,
                                    scores, None)


def workspace(n, N=20109, d=128, k=100, metric=DOT, item_slices=0):
    out = ctypes.c_int64(-1)
    assert lib().bpr_neighbors_workspace(n, N, d, k, metric, item_slices, ctypes.byref(out)) == 0
    return out.value


def plan(n, N, d=128, k=100, metric=DOT, item_slices=0, cus=256):
    fn = lib().bpr_test_neighbors_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 3
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    bounds = (ctypes.c_int64 * 65)()
    assert fn((ctypes.c_int64 * 7)(n, N, d, k, metric, item_slices, cus), out, bounds) == 0
    p = dict(zip(FIELDS, out))
    p["bounds"] = list(bounds[:p["slices"] + 1])
    return p


# ---- arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(X=None), b"NULL"), (dict(T=None), b"NULL"), (dict(rows=None), b"NULL"), (dict(ids=None), b"NULL"),
    (dict(scores=None), b"NULL"), (dict(k=0), b"k must be"), (dict(k=129), b"128"), (dict(d=0), b"d must be"),
    (dict(d=1025), b"1024"), (dict(N=0), b"N in"), (dict(n=-1), b"n must be"), (dict(item_slices=-1), b"item_slices"),
    (dict(item_slices=65), b"item_slices"), (dict(metric=2), b"metric"), (dict(metric=-1), b"metric"),
    (dict(first=-1), b"first"),
    (dict(item_slices=4, N=5000, ws=None, ws_bytes=0), b"workspace"),
    (dict(item_slices=4, N=5000, ws=1, ws_bytes=4 * 4 * 10 * 8 - 1), b"workspace"),
    (dict(metric=COSINE, item_slices=1, ws=None, ws_bytes=0), b"workspace"),  # the norms alone need one
    (dict(metric=COSINE, item_slices=1, ws=1, ws_bytes=(100 + 4) * 4 - 1), b"workspace"),
    (dict(metric=COSINE, item_slices=4, N=5000, ws=1, ws_bytes=4 * 4 * 10 * 8 + (5000 + 4) * 4 - 1), b"workspace"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1  # BPR_ERR_INVALID, bpr_topk_rows' code for each of these
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_queries_is_ok_without_tables():
    assert rows(X=None, T=None, rows=None, ids=None, scores=None, n=0) == 0
    assert rows(X=None, T=None, rows=None, ids=None, scores=None, n=0, k=129) == -1  # (still validated)
    assert rows(X=None, T=None, rows=None, ids=None, scores=None, n=0, metric=7) == -1
    assert rows(n=2 ** 31) == -1 and b"2^31" in lib().bpr_last_error()


def test_workspace_and_slices_refuse_bad_shapes():
    out, s = ctypes.c_int64(), ctypes.c_int32()
    for n, N, d, k, sl in ((4, 100, 8, 0, 0), (4, 100, 8, 129, 0), (4, 100, 0, 10, 0), (4, 100, 1025, 10, 0),
                           (4, 0, 8, 10, 0), (-1, 100, 8, 10, 0), (4, 100, 8, 10, 65), (2 ** 31, 100, 8, 10, 0)):
        assert lib().bpr_neighbors_workspace(n, N, d, k, DOT, sl, ctypes.byref(out)) == -1
        assert lib().bpr_last_error()
        assert lib().bpr_neighbors_slices(n, N, d, k, sl, ctypes.byref(s)) == -1
    assert lib().bpr_neighbors_workspace(4, 100, 8, 10, 2, 0, ctypes.byref(out)) == -1
    assert b"metric" in lib().bpr_last_error()
    assert lib().bpr_neighbors_workspace(4, 100, 8, 10, DOT, 0, None) == -1
    assert lib().bpr_neighbors_slices(4, 100, 8, 10, 0, None) == -1


# ---- plan --------------------------------------------------------------------------------------------------------
def lds_by_hand(k):
    """staged table tile and query tile, the tile's reciprocal norms, then per query: k + 128 candidates of 8 bytes,
    threshold (8), count, pending count, row id, excluded id, reciprocal norm (4 each)"""
    return 4 * (TI + TU) * LD + 4 * TI + TU * ((k + TI) * 8 + 8 + 5 * 4)


@pytest.mark.parametrize("d", [1, 32, 128, 256, 1024])
@pytest.mark.parametrize("metric", [DOT, COSINE])
def test_lds_is_pinned_and_fits_a_cu(d, metric):
    for k, want in ((1, 96_000), (10, 100_608), (100, 146_688), (128, 161_024)):
        p = plan(1000, 20109, d=d, k=k, metric=metric, item_slices=64)
        assert p["lds"] == want == lds_by_hand(k)
        assert p["lds_limit"] == LDS_CU and 0 < p["lds"] <= LDS_CU
        assert p["cap"] == k + TI  # the k best of the last compaction + the most one tile can add
        assert 0 < p["merge_lds"] <= 64 * 1024 + 1024
        assert (p["tile_queries"], p["tile_rows"]) == (TU, TI)


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257, 5000, 20109, 41140, 1_000_003])
def test_slices_cover_the_tiles_exactly_once(N):
    out = ctypes.c_int32(-1)
    for item_slices in (0, 1, 2, 3, 7, 64):
        for n in (1, 1000):
            p = plan(n, N, item_slices=item_slices)
            b = p["bounds"]
            assert b[0] == 0 and b[-1] == N and len(b) == p["slices"] + 1
            assert all(lo < hi for lo, hi in zip(b, b[1:])), b  # disjoint, in order, none empty
            assert all(x % TI == 0 for x in b[:-1])  # whole tiles
            assert p["table_tiles"] == -(-N // TI) and p["query_tiles"] == -(-n // TU)
            assert lib().bpr_neighbors_slices(n, N, 128, 100, item_slices, ctypes.byref(out)) == 0
            assert out.value == p["slices"]


def test_slices_are_the_top_k_kernels():
    """The same (n, N, k) runs with the same slice count through both kernels: what the probe compares."""
    out = ctypes.c_int32(-1)
    for n, N, given in ((1, 20109, 0), (256, 20109, 0), (10_000, 20109, 0), (20_108, 20109, 0), (10_000, 41140, 0),
                        (10_000, 200, 7), (138_493, 20109, 0)):
        assert lib().bpr_topk_slices(n, N, 128, 100, given, ctypes.byref(out)) == 0
        assert plan(n, N, item_slices=given)["slices"] == out.value
    assert plan(1, 20109)["slices"] == 64 and plan(256 * TU, 20109)["slices"] == 1


@pytest.mark.parametrize("metric", [DOT, COSINE])
@pytest.mark.parametrize("k", [1, 100, 128])
def test_workspace_never_shrinks_as_n_grows(metric, k):
    ns = [0, 1, 2, 63, 64, 65, 255, 256, 1000, 4096, 8191, 8192, 10_000, 16_000, 16_320, 16_321, 16_384, 20_000,
          138_493, 571_355]
    got = [workspace(n, k=k, metric=metric, item_slices=0) for n in ns]
    assert all(b >= 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), list(zip(ns, got))
    # ... and it covers the need of the call it is asked for
    for n, w in zip(ns, got):
        assert plan(n, 20109, k=k, metric=metric)["ws_bytes"] <= w


def test_workspace_is_partials_plus_norms():
    """One slice: the kernel writes the result itself.  s slices: s * n * k * 8 bytes of partial results.  Cosine adds
    one fp32 reciprocal norm per table row and per query, (N + n) * 4, and nothing else."""
    N, k = 20109, 100
    for n in (0, 1, 64, 1000, 138_493):
        assert workspace(n, item_slices=1) == 0
        assert workspace(n, metric=COSINE, item_slices=1) == (N + n) * 4
        for s in (2, 7, 64):
            assert workspace(n, item_slices=s) == s * n * k * 8  # (20,109 rows: 158 tiles >= 64 slices)
            assert workspace(n, metric=COSINE, item_slices=s) == s * n * k * 8 + (N + n) * 4
            p = plan(n, N, metric=COSINE, item_slices=s)
            assert (p["partial_bytes"], p["norm_bytes"]) == (s * n * k * 8, (N + n) * 4)
            assert p["ws_bytes"] == p["partial_bytes"] + p["norm_bytes"] == workspace(n, metric=COSINE, item_slices=s)
        assert workspace(n, metric=COSINE) - workspace(n) == (N + n) * 4
        assert plan(n, N, metric=DOT, item_slices=7)["norm_bytes"] == 0
    assert workspace(1000, N=300, metric=COSINE, item_slices=7) == 3 * 1000 * k * 8 + 1300 * 4  # 3 tiles: 3 slices
    # asked with the count a call runs with, the answer is that call's own need
    out = ctypes.c_int32(-1)
    for n in (1, 256, 10_000, 20_108):
        assert lib().bpr_neighbors_slices(n, N, 128, k, 0, ctypes.byref(out)) == 0
        for metric in (DOT, COSINE):
            p = plan(n, N, metric=metric)
            assert workspace(n, metric=metric, item_slices=out.value) == p["ws_bytes"] <= workspace(n, metric=metric)


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_abi_invariants_hold_with_the_three_entry_points():
    """tests/test_abi.py's invariants, restated for the new names: declared in the header, exported, in SIGNATURES
    with the header's argument count; the plan hook is exported but not declared."""
    from revisit_bpr import native

    header = (Path(__file__).resolve().parent.parent / "include" / "bprcore.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(bpr_[a-z_0-9]+)\s*\(", code)))
    assert sorted(native.SIGNATURES) == declared
    for name in ("bpr_neighbors_workspace", "bpr_neighbors_slices", "bpr_neighbors_rows"):
        assert name in declared and hasattr(lib(), name)
        args = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(native.SIGNATURES[name][1]) == args.count(",") + 1
    assert "bpr_test_neighbors_plan" not in declared and hasattr(lib(), "bpr_test_neighbors_plan")
    assert re.search(r"#define\s+BPR_SIM_DOT\s+0\b", code) and re.search(r"#define\s+BPR_SIM_COSINE\s+1\b", code)
    assert (native.SIM_DOT, native.SIM_COSINE) == (0, 1)


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    torch = pytest.importorskip("torch")
    from revisit_bpr.similar import neighbors, similar_items, similar_users

    Q, items = torch.zeros(6, 8), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        neighbors(Q, Q, items, 3)
    with pytest.raises(RuntimeError):
        similar_items(Q, items, 3)
    with pytest.raises(RuntimeError):
        similar_users(Q, items, 3, "dot")
    with pytest.raises(ValueError, match="128"):
        neighbors(Q, Q, items, 129)
    with pytest.raises(ValueError):
        neighbors(Q, Q, items, 0)
    with pytest.raises(ValueError, match="metric"):
        neighbors(Q, Q, items, 3, metric="euclid")
    with pytest.raises(ValueError, match="first"):
        neighbors(Q, Q, items, 3, first=-1)
