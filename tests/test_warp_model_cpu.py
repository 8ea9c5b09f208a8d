"""The WARP objective on the CPU: the numpy model (tests/warp_model.py) against the oracle where the two must
coincide, the statistics of the draw, the share of triples the float32 kernels may decide differently on every
committed input of tests/test_gpu_warp.py, the structured data generator, and the launch plan (bpr_scored_plan.h,
bpr_stream_plan.h) in a program of its own under the host sanitizers."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import counter64_cases as cc
import dynamic_model as dm
import oracle
import warp_cases as wc
import warp_model as wm

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "revisit-bpr_amd" / "csrc"


# ---- 1. N = 1 on all-violating users is the uniform sampler ---------------------------------------------------------
@pytest.mark.parametrize("name", cc.OFFSETS)
def test_one_try_on_a_zero_user_row_is_the_oracles_uniform_sampler_at_64_bit_counters(name):
    pr = wc.problem(40, 90, 16, 30, seed=0, n=64)
    P = np.zeros_like(pr["P"])  # every score 0: every unseen item is within the margin of the positive
    n = len(pr["users"])
    off = cc.offset_of(name, n)
    assert off + n > 2 ** 32
    got, tries, _, _, und, _, _ = wm.sample(P, pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], 1,
                                            wc.MARGIN, cc.SEED, off)
    want = oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"], pr["users"], cc.SEED, off)
    assert np.array_equal(got, want) and (tries == 1).all() and not und.any()
    for broken, where in cc.wrong_streams(lambda u, o: oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"],
                                                                             np.ascontiguousarray(u), cc.SEED, o),
                                          pr["users"], off).values():
        assert (broken[where] != want[where]).mean() > 0.9  # (a wrong counter would show)


def test_the_first_violator_not_the_best_and_nan_rules():
    I, d = 12, 4
    P = np.zeros((2, d), np.float32)
    P[1, 0] = 1.0
    Q = np.zeros((I, d), np.float32)
    Q[1:, 0] = np.arange(1, I)  # score of item a = a
    indptr, indices = np.array([0, 0, 0], np.int64), np.zeros(0, np.int32)
    for t in range(40):
        a = dm.accepted(7, t, set(), I, 8)
        for i, margin in ((6, 1.5), (11, 0.5), (3, 2.5)):  # (no score sits ON a bound: that would be undecided)
            r = wm.draw(7, t, 1, i, 8, margin, P, Q, None, indptr, indices)
            viol = [k for k, c in enumerate(a, 1) if c > i - margin]
            assert r["tries"] == (viol[0] if viol else 0) and r["item"] == (a[viol[0] - 1] if viol else -1)
            assert not r["undecided"] and r["cands"] == a
            if viol:
                assert r["weight"] == math.log(max(1, (I - 1) // viol[0]))
    Qn = Q.copy()
    Qn[5, 1] = np.nan
    for t in range(40):
        r = wm.draw(7, t, 1, 2, 8, 1.0, P, Qn, None, indptr, indices)
        assert r["item"] != 5  # a NaN candidate never violates
        assert wm.draw(7, t, 1, 5, 8, 1.0, P, Qn, None, indptr, indices)["item"] == -1  # a NaN positive skips


# ---- 2. statistics -------------------------------------------------------------------------------------------------------
def test_tries_are_truncated_geometric_and_skips_are_what_is_left():
    """Static scores, one user, N = 6: P(tries = k) = (1 - v)^(k-1) v with v the violating share of the user's unseen
    items, P(skipped) = (1 - v)^N.  Chi-square over 24,000 draws, the skip cell included."""
    Nmax, n, d, I = 6, 24_000, 8, 61
    rng = np.random.default_rng(12)
    P = rng.standard_normal((2, d)).astype(np.float32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    seen_items = np.sort(rng.choice(np.arange(1, I), size=20, replace=False)).astype(np.int32)
    indptr, indices = np.array([0, 0, len(seen_items)], np.int64), seen_items
    unseen = np.array([i for i in range(1, I) if i not in set(seen_items.tolist())])
    s = Q.astype(np.float64) @ P[1].astype(np.float64)
    i_pos = int(unseen[np.argsort(-s[unseen])[11]])  # the positive: 12th best of the 40 unseen items
    margin = 0.25
    v = float((s[unseen] > s[i_pos] - margin).mean())
    assert 0.2 < v < 0.5
    _, tries, _, _, und, _, _ = wm.sample(P, Q, None, indptr, indices, np.full(n, 1, np.int32),
                                          np.full(n, i_pos, np.int32), Nmax, margin, 2024, 0)
    assert not und.any()
    pk, pskip = wm.tries_pmf(v, Nmax)
    assert abs(pk.sum() + pskip - 1) < 1e-12
    obs = np.bincount(tries, minlength=Nmax + 1).astype(np.float64)  # cell 0 = skipped
    exp = np.concatenate([[pskip], pk]) * n
    assert (exp >= 5).all()
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    p = dm.chi2_sf(chi2, len(exp) - 1)
    print(f"v {v:.3f}: skipped {obs[0] / n:.4f} (expected {pskip:.4f}), chi2 {chi2:.2f} over {len(exp)} cells, p = {p:.4g}")
    assert p > 1e-4
    assert abs(obs[0] / n - pskip) < 4 * math.sqrt(pskip * (1 - pskip) / n)


def test_the_substituted_step_is_the_oracles_when_the_weight_is_sigma():
    """warp_model.step with L = sigma(-x) must be oracle.step_sgd_sparse itself; L = 0 leaves the L2 terms."""
    pr = wc.problem(8, 20, 16, 4, seed=1, n=4, bias=True, small=1.0)
    u, i, j = 3, 5, 9
    x = float(pr["P"][u].astype(np.float64) @ (pr["Q"][i] - pr["Q"][j]).astype(np.float64) + pr["b"][i] - pr["b"][j])
    P1, Q1, b1 = pr["P"].copy(), pr["Q"].copy(), pr["b"].copy()
    oracle.step_sgd_sparse(P1, Q1, b1, *(np.array([v], np.int32) for v in (u, i, j)), 0.05, wc.SEQ_REG)
    P2, Q2, b2 = pr["P"].copy(), pr["Q"].copy(), pr["b"].copy()
    wm.step(P2, Q2, b2, u, i, j, 1.0 / (1.0 + math.exp(x)), 0.05, wc.SEQ_REG)
    for a, b in ((P1, P2), (Q1, Q2), (b1, b2)):
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
    P3, Q3, b3 = pr["P"].copy(), pr["Q"].copy(), pr["b"].copy()
    wm.step(P3, Q3, b3, u, i, j, 0.0, 0.05, wc.SEQ_REG)
    assert np.allclose(P3[u], pr["P"][u] * (1 - 0.05 * 0.01), rtol=1e-6) and np.array_equal(b3, pr["b"])
    assert np.allclose(Q3[i], pr["Q"][i] * (1 - 0.05 * 0.02), rtol=1e-6)
    assert np.allclose(Q3[j], pr["Q"][j] * (1 - 0.05 * 0.03), rtol=1e-6)


# ---- 3. the committed inputs of the GPU tests: at most 1 % undecided, and the mix the cases promise --------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", wc.DS)
def test_undecided_share_and_mix_of_the_gpu_pick_cases(d, bias):
    for N in wc.NS:
        items, tries, _, _, und, _, acc = wc.pick_model(N, d, bias)
        print(f"N {N} d {d} bias {bias}: undecided {und.mean():.4%}, skipped {np.mean(tries == 0):.3f}, "
              f"first try {np.mean(tries == 1):.3f}, late {np.mean(tries > max(1, N // 2)):.3f}")
        assert und.mean() <= 0.01 and (acc == N).all()
        assert ((items < 0) == (tries == 0)).all()
        assert (tries == 1).mean() > 0.3
        if N > 1:  # early violators, late violators and skips all occur
            assert (tries == 0).sum() >= 3 and (tries > 1).mean() > 0.02
        if N >= 10:
            assert (tries > 8).any()  # a violator past the first chunk of 8 rows
            assert ((tries == 3) | (tries == 4)).any()  # and in the second chunk of 2 rows, the first of 4 and of 8


def test_undecided_share_of_the_other_gpu_cases():
    for N in (2, 10):
        assert wc.weights_model(N)[4].mean() <= 0.01
    items, tries, _, _, und, _, _ = wc.big_model()
    assert und.mean() <= 0.01 and (tries == 0).any() and (tries > 1).any()
    ed = wc.one_unseen()
    items, tries, _, _, und, _, acc = wm.sample(ed["P"], ed["Q"], None, ed["indptr"], ed["indices"], ed["users"],
                                                ed["pos"], 8, wc.MARGIN, wc.SEED, 0)
    assert not und.any() and (items == ed["unseen"]).all() and (tries == 1).all()
    assert (acc == 0).any() and ((acc > 0) & (acc < 8)).any()


def test_undecided_share_of_the_wide_edge_cases():
    """The d = 1024 runs of the one / none / fewer-than-N unseen case, and the order case's tries."""
    ed = wc.one_unseen(d=1024)
    items, tries, _, _, und, _, acc = wm.sample(ed["P"], ed["Q"], None, ed["indptr"], ed["indices"], ed["users"],
                                                ed["pos"], 8, wc.MARGIN, wc.SEED, 0)
    assert not und.any() and (items == ed["unseen"]).all() and (tries == 1).all()
    assert (acc == 0).any() and ((acc > 0) & (acc < 8)).any()
    few = np.full(len(ed["users"]), 3, np.int32)
    assert wm.sample(ed["P"], ed["Q"], None, ed["indptr"], ed["indices"], few, ed["pos"], 8, wc.MARGIN, wc.SEED,
                     0)[4].mean() <= 0.01
    # the violator of the order case at every place 1 .. 32 and nowhere, at any width (scores are the item ids)
    for d in (32, 512, 1024):
        pr = wc.order_problem(d=d)
        _, tries, _, _, und, _, _ = wm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"],
                                              pr["pos"], 32, 1.5, 5, 0, lists=wc.order_lists())
        assert not und.any() and np.array_equal(np.unique(tries), np.arange(33))
        print(f"d {d}: triples per tries 0 .. 32: {np.bincount(tries).tolist()}")


@pytest.mark.parametrize("d", sorted(wc.dc.GRID_N))
def test_undecided_share_of_the_gpu_grid_windows(d):
    for w in wc.dc.grid_windows(d):
        _, tries, _, _, und, _, acc = wc.grid_model(d, w)
        print(f"d {d} draws {w}: undecided {und.mean():.4%}, triples per tries {np.bincount(tries).tolist()}")
        assert und.mean() <= 0.01 and (acc == wc.GRID_MAX).all()
        assert (tries == 0).any() and (tries > 8).any()  # skips, and a violator past the widest chunk


@pytest.mark.parametrize("d", wc.SEQ_DS)
def test_every_triple_of_the_sequential_cases_is_decided(d):
    P, Q, neg, tries, und, sc = wc.seq_model(d)
    assert not und.any(), int(und.sum())
    assert np.isfinite(P).all() and np.isfinite(Q).all()
    assert sc[3] == (neg >= 0).sum() and 0.1 < (neg < 0).mean() < 0.9 and (tries > 1).any()
    pr = wc.seq_problem(d)
    for u, j in zip(pr["users"], neg):
        assert j == -1 or (j != 0 and j not in pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]])


@pytest.mark.parametrize("d,N", sorted(wc.SEQ_CHUNKED))
def test_every_triple_of_the_chunked_sequential_cases_is_decided(d, N):
    """N over several chunks of four rows: violators in the first chunk, in every later one, and skips."""
    P, Q, neg, tries, und, sc = wc.seq_model(d, N)
    assert not und.any(), int(und.sum())
    assert np.isfinite(P).all() and np.isfinite(Q).all() and sc[3] == (neg >= 0).sum()
    print(f"d {d} N {N}: triples per tries 0 .. {N}: {np.bincount(tries, minlength=N + 1).tolist()}")
    assert (neg < 0).sum() >= 20 and wc.dc.inflight_rows(d) == 4
    for lo in range(0, N, 4):  # a violator in every chunk
        assert ((tries > lo) & (tries <= lo + 4)).sum() >= 5, lo
    pr = wc.seq_problem(d, N)
    for u, j in zip(pr["users"], neg):
        assert j == -1 or (j != 0 and j not in pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]])


def test_the_skip_case_skips_exactly_its_users():
    check_skip_case(32)


def test_the_skip_case_at_sixteen_entries_a_lane_skips_exactly_its_users():
    check_skip_case(640)  # (a width at which the model leaves no triple of the case undecided)


def check_skip_case(d):
    pr = wc.skip_problem(d)
    P, Q, b, neg, tries, und, sc = wc.skip_model(10, d)
    sk = np.isin(pr["users"], pr["skipped"])
    assert not und.any() and sk.sum() >= 20 and (neg[sk] == -1).all() and (neg[~sk] >= 0).mean() > 0.5
    assert np.array_equal(P[pr["skipped"]], pr["P"][pr["skipped"]]) and np.array_equal(Q[pr["top"]], pr["Q"][pr["top"]])
    assert b[pr["top"]] == pr["b"][pr["top"]] and sc[3] == (neg >= 0).sum()


# ---- 4. data with per-user structure ------------------------------------------------------------------------------------
def test_generate_structured():
    from revisit_bpr.datasets import synthetic

    a = synthetic.generate_structured(200, 300, 6000, seed=4)
    b = synthetic.generate_structured(200, 300, 6000, seed=4)
    c = synthetic.generate_structured(200, 300, 6000, seed=5)
    for k in ("users", "items", "indptr", "indices", "eval_users", "eval_indptr", "eval_items"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(c, k).dtype
    assert not np.array_equal(a.items, c.items)
    assert a.num_users == 201 and a.num_items == 301 and 0.8 * 6000 <= a.nnz <= 1.2 * 6000
    assert a.users.dtype == np.int32 and a.indptr.dtype == np.int64 and a.indptr[-1] == a.nnz and a.indptr[1] == 0
    key = a.users.astype(np.int64) * a.num_items + a.items
    assert len(np.unique(key)) == a.nnz and a.items.min() >= 1 and a.users.min() >= 1 and a.items.max() <= 300
    assert np.array_equal(a.indices, a.items) and (np.diff(a.users) >= 0).all()
    # item popularity follows the skew: the count of an item rises with the popularity it was drawn with, and more so
    # at a larger skew
    A, B, logpop = synthetic.structured_factors(200, 300, 6000, seed=4)

    def pop_corr(data):
        cnt = np.bincount(data.items, minlength=301)[1:].astype(np.float64)
        r = lambda x: np.argsort(np.argsort(x)).astype(np.float64)
        return float(np.corrcoef(r(cnt), r(logpop[1:]))[0, 1])

    flat = synthetic.generate_structured(200, 300, 6000, seed=4, popularity_skew=0.0)
    steep = synthetic.generate_structured(200, 300, 6000, seed=4, popularity_skew=2.0)
    print(f"rank correlation of item count with popularity: skew 0 {pop_corr(flat):.3f}, 1 {pop_corr(a):.3f}, "
          f"2 {pop_corr(steep):.3f}")
    assert abs(pop_corr(flat)) < 0.2 and pop_corr(a) > 0.5 and pop_corr(steep) > pop_corr(a)
    # a user's items score above its non-items on the generating factors
    s = A @ B.T
    aucs = []
    for u in range(1, 201):
        mine = a.indices[a.indptr[u]:a.indptr[u + 1]]
        rest = np.setdiff1d(np.arange(1, 301), mine)
        if len(mine):
            aucs.append(float((s[u, mine][:, None] > s[u, rest][None, :]).mean()))
    print(f"AUC of the generating factors: {np.mean(aucs):.3f}")
    assert np.mean(aucs) > 0.65
    # a hold-out, as generate_named's
    e = synthetic.generate_structured(200, 300, 6000, seed=4, eval_users=50)
    assert len(e.eval_users) == 50 and e.eval_indptr[-1] == len(e.eval_items) > 0 and e.nnz + len(e.eval_items) == a.nnz
    with pytest.raises(ValueError):
        synthetic.generate_structured(10, 30, 100, temperature=0.0)


# ---- 5. the plan ----------------------------------------------------------------------------------------------------------
def test_plan_headers_alone_under_the_host_sanitizers(tmp_path):
    """bpr_scored_plan.h and bpr_stream_plan.h are plain C++: built into a program of its own with
    -fsanitize=address,undefined, tests/warp_plan_check.cpp runs clean."""
    exe = tmp_path / "warp_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "warp_plan_check.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 6. the C ABI refuses before it touches a device --------------------------------------------------------------------
def test_abi_refusals_need_no_device():
    from revisit_bpr import native

    lib = native.load()
    assert native.NEG_WARP == 4
    assert lib.bpr_set_warp(None, 10, 1.0) == -1 and b"NULL" in lib.bpr_last_error()
    assert lib.bpr_sample_warp(None, None, None, 0, 10, 1.0, 0, 0, None, None, None, None) == -1
    assert lib.bpr_train_strict(None, None, None, None, 0, 1, 4, 0.5, 0, 0, 0, None) == -3
    assert b"WARP" in lib.bpr_last_error()
    assert lib.bpr_train_stream_batched(None, None, None, None, 0, 1, 4, 0.5, 0, 0, 0, None) == -3
    assert b"WARP" in lib.bpr_last_error()
    assert lib.bpr_train_stream_acut(None, None, None, None, 1, 4, 0.5, 0, 0, 0, None) == -3
    assert b"WARP" in lib.bpr_last_error()
    assert lib.bpr_step(None, None, None, None, 0, native.MODE_STRICT, 4, 0.5, 0, 0, None, None, None) == -3
    assert b"WARP" in lib.bpr_last_error()
    assert lib.bpr_fold_in_rows(None, None, 10, 8, None, None, 1, None, 1, 0.1, 0.0, 4, None, None, 0, 0, None,
                                None) == -3
    assert b"WARP" in lib.bpr_last_error()


def test_schedule_and_trainers_take_the_new_name():
    from revisit_bpr import fast

    u = fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="uniform", hot_lds=0)
    w = fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="warp")
    assert w == u and w.hot_lds == 0 and w.refresh_lag == 0.0 and w.refresh_cus == 0
    with pytest.raises(ValueError, match="LDS tier"):
        fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="warp", hot_lds=64)
    with pytest.raises(ValueError, match="plain-SGD STREAM kernel only"):
        fast._refuse_warp("warp", "BatchedStreamTrainer")
    fast._refuse_warp("uniform", "StrictTrainer")
    fast._refuse_warp("dynamic", "StrictTrainer")
