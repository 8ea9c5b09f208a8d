"""Diversified top-k on a machine without a GPU: the numpy model of the contract (tests/diversify_model.py) pinned
against an independent torch statement, the launch plan (revisit-bpr_amd/csrc/bpr_diversify_plan.h — through the
library's test hook, and alone in a host program built under the host sanitizers), the argument validation of
`bpr_diversify_rows` / `bpr_diversify_layout` (nothing touches the device before the arguments are checked) and the
Python wrapper's refusals."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from diversify_model import chain_dot, diversify_rows, sim_matrix

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
LDS_CU = 163_840
FIELDS = ("layout", "cpad", "tiles", "grid", "lds", "lds_limit", "grid_max", "threads", "cmax")


def lib():
    from revisit_bpr import native

    return native.load()


# ---- 1. the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("scale", ["none", "minmax"])
def test_model_against_a_torch_statement(metric, scale):
    """float64 Gram on an integer table (exact), float32 only where the contract rounds, then the greedy loop as a
    sort by the key per step"""
    torch = pytest.importorskip("torch")
    I, d, C, k = 40, 12, 17, 9
    g = np.random.default_rng(3)
    Q = g.integers(-3, 4, (I, d)).astype(np.float32)
    Q[7] = 0
    Q[9] = Q[8]
    assert np.array_equal(chain_dot(Q, Q), (Q.astype(np.float64) @ Q.T.astype(np.float64)).astype(np.float32))
    S = sim_matrix(Q, metric)
    assert np.array_equal(S, S.T) and not S[7].any()
    Qt = torch.from_numpy(Q).double()
    Gt = (Qt @ Qt.T).float()
    if metric == "cosine":
        ss = torch.diagonal(Gt)
        rn = torch.where(ss > 0, 1.0 / torch.sqrt(ss), torch.zeros(()))
        St = Gt * (rn[:, None] * rn[None, :])
        St[ss <= 0, :] = 0
        St[:, ss <= 0] = 0
    else:
        St = Gt
    assert np.array_equal(St.numpy(), S)
    ci = g.integers(-2, I + 2, (12, C)).astype(np.int32)
    cs = (g.integers(-8, 9, (12, C)) / 4).astype(np.float32)
    cs[0, :3] = [np.nan, np.inf, -np.inf]
    ci[1] = -1
    ci[2, :3], cs[2, :3] = 5, [1.0, 1.0, 0.5]
    total_ties = 0
    for lam in (0.0, 0.5, 0.75, 1.0):
        items, scores, mmr, ties = diversify_rows(S, ci, cs, k, lam, scale)
        total_ties += ties
        lam32 = torch.tensor(lam, dtype=torch.float32)
        for r in range(ci.shape[0]):
            pool = [(int(i), float(s), p) for p, (i, s) in enumerate(zip(ci[r], cs[r])) if 0 < i < I and np.isfinite(s)]
            rel = torch.tensor([p[1] for p in pool], dtype=torch.float32)
            relp = rel
            if scale == "minmax" and pool:
                relp = torch.zeros_like(rel) if rel.max() == rel.min() else (rel - rel.min()) / (rel.max() - rel.min())
            m = torch.zeros(len(pool))
            got = []
            left = list(range(len(pool)))
            for step in range(min(k, len(pool))):
                v = lam32 * relp - (1 - lam32) * m
                best = sorted(left, key=lambda c: (-float(v[c]), -pool[c][1], pool[c][0], pool[c][2]))[0]
                got.append((pool[best][0], pool[best][1], float(v[best])))
                left.remove(best)
                sim = St[[p[0] for p in pool], pool[best][0]]
                m = sim if step == 0 else torch.maximum(m, sim)
            want_i = [x[0] for x in got] + [-1] * (k - len(got))
            want_s = [x[1] for x in got] + [-np.inf] * (k - len(got))
            want_v = [x[2] for x in got] + [-np.inf] * (k - len(got))
            assert items[r].tolist() == want_i and scores[r].tolist() == want_s and mmr[r].tolist() == want_v, (lam, r)
    assert total_ties > 20  # the data does hold what it is meant to
    items1, scores1, _, _ = diversify_rows(S, ci[3], cs[3], k, 1.0, "none")  # lam = 1: (score desc, id asc)
    pool = sorted((-float(s), int(i)) for i, s in zip(ci[3], cs[3]) if 0 < i < I and np.isfinite(s))[:k]
    assert items1[0, :len(pool)].tolist() == [p[1] for p in pool]


# ---- 2. the plan -------------------------------------------------------------------------------------------------
def plan(n, C=100, k=10, layout=0):
    fn = lib().bpr_test_diversify_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 2
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn((ctypes.c_int64 * 4)(n, C, k, layout), out) == 0, lib().bpr_last_error()
    return dict(zip(FIELDS, out))


@pytest.mark.parametrize("C", [1, 31, 32, 33, 64, 65, 96, 97, 127, 128])
def test_lds_fits_a_cu_for_every_pool(C):
    """Gram tiles on or above the diagonal ([32][33] floats each), one staged chunk [cpad][36], three words per
    candidate, 128 bytes of exchange and scalars: whatever d and k"""
    cpad = -(-C // 32) * 32
    T = cpad // 32
    for k in (0, 1, 128):
        p = plan(1000, C=C, k=k)
        assert (p["cpad"], p["tiles"], p["threads"], p["cmax"]) == (cpad, T * (T + 1) // 2, 256, 128)
        assert p["lds"] == 4 * p["tiles"] * 32 * 33 + 4 * cpad * 36 + 12 * cpad + 128
        assert p["lds_limit"] == LDS_CU and 0 < p["lds"] <= 65_536 <= LDS_CU
    assert [plan(1, C=c)["lds"] for c in (32, 64, 96, 128)] == [9_344, 22_784, 40_448, 62_336]
    assert 2 * plan(1, C=128)["lds"] <= LDS_CU and 7 * plan(1, C=64)["lds"] <= LDS_CU  # short pools share a CU


def test_layout_choice_and_forcing():
    from revisit_bpr import diversify

    assert (diversify.LAYOUT_AUTO, diversify.LAYOUT_WG, diversify.LAYOUTS, diversify.POOL_MAX) == (0, 1, (1,), 128)
    for n in (1, 70, 10_000, 2 ** 31 + 5):
        for C in (1, 32, 33, 100, 128):
            for layout in (0, 1):
                p = plan(n, C=C, layout=layout)
                assert p["layout"] == 1
                assert diversify.layout_of(n, C, 10, layout) == (1, p["cpad"], p["lds"])


@pytest.mark.parametrize("n", [0, 1, 70, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 22 + 1, 2 ** 31 + 5])
def test_grid_covers_the_rows_and_does_not_overflow(n):
    p = plan(n)
    assert p["grid"] == min(n, p["grid_max"]) and p["grid_max"] == 2 ** 20
    assert p["grid"] * 256 < 2 ** 32  # HIP's bound on grid x block
    assert (p["grid"] > 0) == (n > 0)  # (a workgroup walks rows r, r + grid, ...: every row once)


def test_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """bpr_diversify_plan.h is plain C++: built into a program of its own with -fsanitize=address,undefined, its
    sweep (tests/diversify_plan_check.cpp: every pool length, row counts past 2^31) runs clean."""
    exe = tmp_path / "diversify_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "diversify_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 3. arguments ------------------------------------------------------------------------------------------------
def rows(Q=1, I=100, d=8, citems=1, cscores=1, n=4, C=10, k=5, lam=0.7, metric=1, scale=0, layout=0, items=1, scores=1,
         mmr=None):
    """bpr_diversify_rows with fake non-NULL pointers (1) where a pointer is wanted: only calls that must be refused
    before the device is touched, or n = 0 / k = 0, go through here."""
    return lib().bpr_diversify_rows(Q, I, d, citems, cscores, n, C, k, lam, metric, scale, layout, items, scores, mmr,
                                    None)


@pytest.mark.parametrize("kw, word", [
    (dict(Q=None), b"NULL"), (dict(citems=None), b"NULL"), (dict(cscores=None), b"NULL"), (dict(items=None), b"NULL"),
    (dict(scores=None), b"NULL"), (dict(C=129), b"C must be"), (dict(C=0), b"C must be"), (dict(k=129), b"k must be"),
    (dict(k=-1), b"k must be"), (dict(lam=-0.1), b"lam"), (dict(lam=1.5), b"lam"), (dict(lam=float("nan")), b"lam"),
    (dict(d=0), b"d must be"), (dict(d=1025), b"1024"), (dict(I=0), b"I must be"), (dict(I=2 ** 31), b"I must be"),
    (dict(n=-1), b"n must be"), (dict(metric=2), b"metric"), (dict(metric=-1), b"metric"), (dict(scale=2), b"scale"),
    (dict(layout=2), b"layout"), (dict(layout=-1), b"layout"),
])
def test_bad_arguments_are_refused_with_a_message(kw, word):
    assert rows(**kw) == -1  # BPR_ERR_INVALID
    assert word in lib().bpr_last_error(), lib().bpr_last_error()


def test_no_rows_is_ok_without_tables():
    none = dict(Q=None, citems=None, cscores=None, items=None, scores=None)
    assert rows(n=0, **none) == 0
    assert rows(k=0, **none) == 0
    assert rows(n=0, k=129, **none) == -1  # (still validated)
    assert rows(n=0, lam=1.5, **none) == -1
    lay, cpad, lds = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    refs = (ctypes.byref(lay), ctypes.byref(cpad), ctypes.byref(lds))
    assert lib().bpr_diversify_layout(4, 10, 5, 0, None, refs[1], refs[2]) == -1
    assert lib().bpr_diversify_layout(4, 129, 5, 0, *refs) == -1
    assert lib().bpr_diversify_layout(4, 10, 129, 0, *refs) == -1
    assert lib().bpr_diversify_layout(4, 10, 5, 2, *refs) == -1
    assert lib().bpr_diversify_layout(2 ** 31 + 5, 100, 10, 0, *refs) == 0
    assert (lay.value, cpad.value, lds.value) == (1, 128, 62_336)


def test_abi_invariants_hold_with_the_two_entry_points():
    from revisit_bpr import native

    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bprcore.h").read_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bpr_[a-z_0-9]+)\s*\(", code)))
    assert sorted(native.SIGNATURES) == declared
    for name in ("bpr_diversify_rows", "bpr_diversify_layout"):
        assert name in declared and hasattr(lib(), name)
        args = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(native.SIGNATURES[name][1]) == args.count(",") + 1
    assert "bpr_test_diversify_plan" not in declared and hasattr(lib(), "bpr_test_diversify_plan")
    assert re.search(r"#define\s+BPR_SCALE_NONE\s+0", code) and re.search(r"#define\s+BPR_SCALE_MINMAX\s+1", code)


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    torch = pytest.importorskip("torch")
    from revisit_bpr.diversify import diversify, intra_list_similarity, recommend_diverse

    Q = torch.zeros(6, 8)
    ci, cs = torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        diversify(Q, ci, cs, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        diversify(Q, ci[0], cs[0], 3, return_mmr=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        recommend_diverse(torch.zeros(4, 8), Q, None, torch.zeros(2, dtype=torch.int32), 3, pool=5)
    with pytest.raises(ValueError, match="128"):
        diversify(Q, ci, cs, 129)
    with pytest.raises(ValueError, match="128"):
        diversify(Q, torch.ones(2, 129, dtype=torch.int32), torch.zeros(2, 129), 3)
    with pytest.raises(ValueError, match="at least 0"):
        diversify(Q, ci, cs, -1)
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            diversify(Q, ci, cs, 3, lam=lam)
    with pytest.raises(ValueError, match="float32"):
        diversify(Q.double(), ci, cs, 3)
    with pytest.raises(ValueError, match="cand_items must be int32"):
        diversify(Q, ci.long(), cs, 3)
    with pytest.raises(ValueError, match="cand_scores must be float32"):
        diversify(Q, ci, cs.double(), 3)
    with pytest.raises(ValueError, match="same shape"):
        diversify(Q, ci, cs[:, :4], 3)
    with pytest.raises(ValueError, match="1-D"):
        diversify(Q, ci.reshape(1, 2, 5), cs.reshape(1, 2, 5), 3)
    with pytest.raises(ValueError, match="metric"):
        diversify(Q, ci, cs, 3, metric="l2")
    with pytest.raises(ValueError, match="scale"):
        diversify(Q, ci, cs, 3, scale="zscore")
    with pytest.raises(ValueError, match="layout"):
        diversify(Q, ci, cs, 3, layout=2)
    with pytest.raises(ValueError, match="pool"):
        recommend_diverse(torch.zeros(4, 8), Q, None, torch.zeros(2, dtype=torch.int32), 3, pool=129)
    with pytest.raises(ValueError, match="pool"):
        recommend_diverse(torch.zeros(4, 8), Q, None, torch.zeros(2, dtype=torch.int32), 6, pool=5)
    # the metric is plain torch and runs anywhere: two orthogonal rows and a copy of the first
    T = torch.tensor([[0.0, 0.0], [2.0, 0.0], [0.0, 3.0], [5.0, 0.0]])
    ils = intra_list_similarity(T, torch.tensor([[1, 2, -1], [1, 3, -1], [1, -1, -1], [1, 2, 3]]))
    assert torch.allclose(ils, torch.tensor([0.0, 1.0, 0.0, 1 / 3]))
    assert torch.allclose(intra_list_similarity(T, torch.tensor([1, 3]), "dot"), torch.tensor([10.0]))
