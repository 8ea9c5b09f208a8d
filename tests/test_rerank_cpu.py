"""Re-ranking on a machine without a GPU: the numpy model of the contract (tests/rerank_model.py) pinned against an
independent torch statement, the launch plan (revisit-bpr_amd/csrc/bpr_rerank_plan.h — through the library's test
hook, and alone in a host program built under the host sanitizers), the argument validation of `bpr_rerank_rows` /
`bpr_rerank_layout` (nothing touches the device before the arguments are checked) and the Python wrapper's refusals."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rerank_model import rerank_rows

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
LDS_CU = 163_840
WAVE, WG = 1, 2
FIELDS = ("layout", "tile", "rows_per_group", "cap", "groups", "grid", "team_lds", "lds", "lds_limit", "wave_max_len",
          "grid_max", "wave_mid_len", "wave_mid_rows", "wave_any_rows")


def lib():
    from revisit_bpr import native

    return native.load()


# ---- 1. the model ------------------------------------------------------------------------------------------------
def test_model_against_a_torch_statement():
    """gather, -inf mask, stable sort by (-score, id) — on exact tables, so that ties are plentiful"""
    torch = pytest.importorskip("torch")
    U, I, d, k = 6, 40, 8, 7
    g = np.random.default_rng(5)
    P = (g.integers(-4, 5, (U, d)) / 4).astype(np.float32)
    Q = (g.integers(-4, 5, (I, d)) / 4).astype(np.float32)
    b = (g.integers(-8, 9, I) / 4).astype(np.float32)
    S = (P.astype(np.float64) @ Q.T.astype(np.float64) + b).astype(np.float32)
    seen = [np.sort(g.choice(np.arange(1, I), g.integers(0, 12), replace=False)).astype(np.int32) for _ in range(U)]
    seen[1] = np.arange(1, I, dtype=np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64)
    indices = np.concatenate(seen).astype(np.int32)
    users = np.array([0, 1, 2, 3, 4, 5, 2, 0], np.int32)
    rows = [g.integers(-2, I + 3, g.integers(0, 30)).astype(np.int32) for _ in users]  # ids out of range, duplicates
    rows[2] = np.array([5, 9, 5, 0, 5, I, -3, 9], np.int32)
    rows[3] = np.zeros(0, np.int32)
    cptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    citems = np.concatenate(rows).astype(np.int32)
    ties = dups = short = 0
    for csr in (True, False):
        items, scores, cand = rerank_rows(S, users, cptr, citems, k, *((indptr, indices) if csr else (None, None)))
        for r, u in enumerate(users):
            c = torch.from_numpy(citems[cptr[r]:cptr[r + 1]]).long()
            ok = (c > 0) & (c < I)
            if csr:
                ok &= ~torch.isin(c, torch.from_numpy(seen[u]).long())
            s = torch.where(ok, torch.from_numpy(S)[int(u), c.clamp(0, I - 1)], torch.tensor(-np.inf))
            assert np.array_equal(cand[cptr[r]:cptr[r + 1]], s.numpy())
            order = torch.argsort(c, stable=True)          # by id ...
            order = order[torch.argsort(-s[order], stable=True)]  # ... then, stably, by score descending
            order = order[ok[order]][:k]
            want_i = np.full(k, -1, np.int32)
            want_s = np.full(k, -np.inf, np.float32)
            want_i[:len(order)], want_s[:len(order)] = c[order].numpy(), s[order].numpy()
            assert np.array_equal(items[r], want_i) and np.array_equal(scores[r], want_s), (csr, r)
            live = scores[r][items[r] >= 0]
            ties += int((np.diff(live) == 0).sum())
            dups += int((np.diff(items[r][items[r] >= 0]) == 0).sum())
            short += int((items[r] < 0).any())
        if csr:
            assert (items[1] == -1).all() and np.isneginf(cand[cptr[1]:cptr[2]]).all()  # everything seen
    assert ties > 5 and dups > 2 and short > 2  # the data does hold what it is meant to
    # the shared list is the CSR with the list repeated
    L = rows[2]
    a = rerank_rows(S, users, None, L, k, indptr, indices)
    rep = np.arange(len(users) + 1, dtype=np.int64) * len(L)
    b2 = rerank_rows(S, users, rep, np.tile(L, len(users)), k, indptr, indices)
    assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1])
    assert np.array_equal(a[2].reshape(-1), b2[2]) and a[2].shape == (len(users), len(L))


# ---- 2. the plan -------------------------------------------------------------------------------------------------
def plan(n, d=128, k=10, row_len=0, layout=0):
    fn = lib().bpr_test_rerank_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 5)(n, d, k, row_len, layout), out) == 0, lib().bpr_last_error()
    return dict(zip(FIELDS, out))


def team_lds_by_hand(tile, d, k):
    """the staged tile, P[u] padded to 32 floats, the tile's ids, k + tile candidates of 12 bytes, the threshold (12),
    count and pending count (4 each); rounded up to 16"""
    b = 4 * tile * 36 + 4 * (-(-d // 32) * 32) + 4 * tile + (k + tile) * 12 + 12 + 8
    return -(-b // 16) * 16


@pytest.mark.parametrize("d", [1, 33, 128, 256, 1024])
@pytest.mark.parametrize("k", [0, 1, 10, 128])
def test_lds_fits_a_cu_for_every_layout(d, k):
    for layout, tile, rows in ((WAVE, 64, 4), (WG, 256, 1)):
        p = plan(1000, d=d, k=k, row_len=500, layout=layout)
        assert (p["layout"], p["tile"], p["rows_per_group"], p["cap"]) == (layout, tile, rows, k + tile)
        assert p["team_lds"] == team_lds_by_hand(tile, d, k) and p["lds"] == rows * p["team_lds"]
        assert p["lds_limit"] == LDS_CU and 0 < p["lds"] <= 65_536 <= LDS_CU
    assert plan(1, d=1024, k=128, layout=WAVE)["lds"] == 63_616
    assert plan(1, d=1024, k=128, layout=WG)["lds"] == 46_624


def test_layout_choice_and_forcing():
    from revisit_bpr import rerank

    c = plan(10)
    t, mid, rows_mid, rows_any = c["wave_max_len"], c["wave_mid_len"], c["wave_mid_rows"], c["wave_any_rows"]
    assert (t, mid, rows_mid, rows_any) == (128, 1024, 1024, 8192)
    lengths = list(range(0, 2 * t + 2)) + [mid - 1, mid, mid + 1, 20_109, 2 ** 40]
    for n in (1, 10, rows_mid - 1, rows_mid, rows_mid + 1, rows_any - 1, rows_any, rows_any + 1, 2 ** 31 + 5):
        for length in lengths:
            # short lists always; middling ones once the rows fill the chip; any list (0: a CSR whose rows the plan
            # knows nothing about) once there are rows enough
            want = WAVE if 1 <= length <= t or (1 <= length <= mid and n >= rows_mid) or n >= rows_any else WG
            p = plan(n, row_len=length)
            assert p["layout"] == want and p["tile"] == (64 if want == WAVE else 256), (n, length)
            for forced in (WAVE, WG):
                assert plan(n, row_len=length, layout=forced)["layout"] == forced
            assert rerank.layout_of(n, 128, 10, length) == (p["layout"], p["tile"])
    assert rerank.RERANK_TILE == 256 == max(plan(1, layout=WAVE)["tile"], plan(1, layout=WG)["tile"])
    assert (rerank.LAYOUT_WAVE, rerank.LAYOUT_WG, rerank.LAYOUTS) == (WAVE, WG, (WAVE, WG))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 70, 2 ** 20, 2 ** 20 + 1, 2 ** 22 + 1, 2 ** 31 + 5])
def test_grid_covers_the_rows_and_does_not_overflow(n):
    for layout, rows in ((WAVE, 4), (WG, 1)):
        p = plan(n, layout=layout)
        assert p["groups"] == -(-n // rows)
        assert p["grid"] == min(p["groups"], p["grid_max"]) and p["grid_max"] == 2 ** 20
        assert p["grid"] * 256 < 2 ** 32  # HIP's bound on grid x block
        assert (p["grid"] > 0) == (n > 0)  # (a workgroup walks groups g, g + grid, ...: every group once)


def test_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """bpr_rerank_plan.h is plain C++: built into a program of its own with -fsanitize=address,undefined, its sweep
    (tests/rerank_plan_check.cpp: row counts past 2^31, every length around the threshold) runs clean."""
    exe = tmp_path / "rerank_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "rerank_plan_check.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3. arguments ------------------------------------------------------------------------------------------------
def rows(P=1, Q=1, bias=None, I=100, d=8, users=1, n=4, cptr=1, citems=1, shared_len=0, sptr=None, sidx=None, k=10,
         layout=0, cand=None, items=1, scores=1):
    """bpr_rerank_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0, go through here."""
    return lib().bpr_rerank_rows(P, Q, bias, I, d, users, n, cptr, citems, shared_len, sptr, sidx, k, layout, cand,
                                 items, scores, None)


@pytest.mark.parametrize("kw, word", [
    (dict(P=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(users=None), b"NULL"), (dict(citems=None), b"cand_items"),
    (dict(cptr=None, citems=None, shared_len=5), b"cand_items"), (dict(items=None), b"NULL"),
    (dict(scores=None), b"NULL"), (dict(k=129), b"128"), (dict(k=-1), b"k must be"),
    (dict(k=0, cand=None), b"cand_scores_out"), (dict(d=0), b"d must be"), (dict(d=1025), b"1024"),
    (dict(I=0), b"I must be"), (dict(I=2 ** 31), b"I must be"), (dict(n=-1), b"n must be"),
    (dict(shared_len=-1), b"length"), (dict(layout=3), b"layout"), (dict(layout=-1), b"layout"),
    (dict(sptr=1), b"go together"), (dict(sidx=1), b"go together"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1  # BPR_ERR_INVALID
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_rows_is_ok_without_tables():
    assert rows(P=None, Q=None, users=None, cptr=None, citems=None, items=None, scores=None, n=0) == 0
    assert rows(P=None, Q=None, users=None, cptr=None, citems=None, items=None, scores=None, n=0, k=129) == -1
    assert rows(P=None, Q=None, users=None, n=0, k=0, cand=None) == -1  # (still validated)
    lay, tile = ctypes.c_int32(), ctypes.c_int32()
    assert lib().bpr_rerank_layout(4, 8, 10, 5, 0, None, ctypes.byref(tile)) == -1
    assert lib().bpr_rerank_layout(4, 8, 129, 5, 0, ctypes.byref(lay), ctypes.byref(tile)) == -1
    assert lib().bpr_rerank_layout(4, 8, 10, 5, 3, ctypes.byref(lay), ctypes.byref(tile)) == -1
    assert lib().bpr_rerank_layout(2 ** 31 + 5, 8, 10, 5, 0, ctypes.byref(lay), ctypes.byref(tile)) == 0
    assert (lay.value, tile.value) == (WAVE, 64)


def test_abi_invariants_hold_with_the_two_entry_points():
    from revisit_bpr import native

    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bprcore.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bpr_[a-z_0-9]+)\s*\(", code)))
    assert sorted(native.SIGNATURES) == declared
    for name in ("bpr_rerank_rows", "bpr_rerank_layout"):
        assert name in declared and hasattr(lib(), name)
        args = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(native.SIGNATURES[name][1]) == args.count(",") + 1
    assert "bpr_test_rerank_plan" not in declared and hasattr(lib(), "bpr_test_rerank_plan")


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    torch = pytest.importorskip("torch")
    from revisit_bpr.rerank import rerank, score_candidates

    P, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    users, cand = torch.zeros(2, dtype=torch.int32), torch.ones(5, dtype=torch.int32)
    cptr = torch.tensor([0, 2, 5])
    with pytest.raises(RuntimeError, match="ROCm device"):
        rerank(P, Q, None, users, cand, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        rerank(P, Q, None, users, cand, 3, cptr, return_scores=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        score_candidates(P, Q, None, users, cand)
    with pytest.raises(ValueError, match="128"):
        rerank(P, Q, None, users, cand, 129)
    with pytest.raises(ValueError, match="return_scores"):
        rerank(P, Q, None, users, cand, 0)
    with pytest.raises(ValueError, match="at least 0"):
        rerank(P, Q, None, users, cand, -1)
    with pytest.raises(ValueError, match="float32"):
        rerank(P.double(), Q, None, users, cand, 3)
    with pytest.raises(ValueError, match="float32"):
        rerank(P, Q, torch.zeros(6, dtype=torch.float64), users, cand, 3)
    with pytest.raises(ValueError, match="cand_items must be int32"):
        rerank(P, Q, None, users, cand.long(), 3)
    with pytest.raises(ValueError, match="users must be"):
        rerank(P, Q, None, users.float(), cand, 3)
    with pytest.raises(ValueError, match="cand_indptr must be int64"):
        rerank(P, Q, None, users, cand, 3, cptr.int())
    with pytest.raises(ValueError, match="n\\+1"):
        rerank(P, Q, None, users, cand, 3, torch.tensor([0, 5]))
    with pytest.raises(ValueError, match="n\\+1"):
        score_candidates(P, Q, None, users, cand, torch.tensor([0, 1, 2, 5]))
    with pytest.raises(ValueError, match="1-D"):
        rerank(P, Q, None, users, cand.reshape(1, 5), 3)
    with pytest.raises(ValueError, match="one entry per item"):
        rerank(P, Q, torch.zeros(5), users, cand, 3)
    with pytest.raises(ValueError, match="go together"):
        rerank(P, Q, None, users, cand, 3, seen_indptr=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="layout"):
        rerank(P, Q, None, users, cand, 3, layout=3)
