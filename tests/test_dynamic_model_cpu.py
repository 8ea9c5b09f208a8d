"""Dynamic negative sampling on the CPU: the numpy model (tests/dynamic_model.py) against the oracle where the two
must coincide, the statistics of the pick, the share of triples the float32 kernels may decide differently on every
committed input of tests/test_gpu_dynamic.py, and the launch plan (bpr_scored_plan.h, bpr_stream_plan.h) in a program
of its own under the host sanitizers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import counter64_cases as cc
import dynamic_cases as dc
import dynamic_model as dm
import oracle

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "revisit-bpr_amd" / "csrc"


def small(U=40, I=90, per_user=30, seed=0, n=256):
    pr = dc.problem(U, I, 16, per_user, seed, n)
    return pr


# ---- 1. where the model must be the uniform sampler --------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.OFFSETS)
def test_one_candidate_is_the_oracles_uniform_sampler_at_64_bit_counters(name):
    """M = 1 on the counter-64 list (tests/counter64_cases.py: the carry into the high word inside the call, a rank's
    offset, both), with the 64-bit seed."""
    pr = small(n=64)
    n = len(pr["users"])
    off = cc.offset_of(name, n)
    assert off + n > 2 ** 32
    got, _, dec, _, _ = dm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], 1, cc.SEED, off)
    want = oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"], pr["users"], cc.SEED, off)
    assert np.array_equal(got, want) and dec.all()
    for broken, where in cc.wrong_streams(lambda u, o: oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"],
                                                                             np.ascontiguousarray(u), cc.SEED, o),
                                          pr["users"], off).values():
        assert (broken[where] != want[where]).mean() > 0.9  # (a wrong counter would show)


def test_one_candidate_with_item_weights_is_the_oracles_weighted_sampler():
    pr = small(n=200, seed=4)
    w = np.random.default_rng(1).random(pr["I"]) ** 3
    accept, alias = oracle.alias_table(w)
    got, _, _, _, _ = dm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], 1, 11, 2 ** 32 + 5,
                                accept, alias)
    want = oracle.sample_weighted(pr["indptr"], pr["indices"], pr["I"], pr["users"], 11, 2 ** 32 + 5, accept, alias)
    assert np.array_equal(got, want)


def test_a_zero_user_row_is_the_uniform_sampler_at_any_m():
    pr = small(n=200, seed=2)
    P = pr["P"].copy()
    P[:] = 0
    got, sc, dec, _, _ = dm.sample(P, pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], 8, 5, 77)
    assert np.array_equal(got, oracle.sample_uniform(pr["indptr"], pr["indices"], pr["I"], pr["users"], 5, 77))
    assert dec.all() and not sc.any()


def test_the_rank_pick_is_the_oracles():
    """A user who has seen all but one item: most triples accept no candidate and take the oracle's exact pick."""
    e = dc.nearly_all_seen()
    got, _, dec, _, acc = dm.sample(e["P"], e["Q"], None, e["indptr"], e["indices"], e["users"], 8, dc.SEED, 0)
    want = oracle.sample_uniform(e["indptr"], e["indices"], e["I"], e["users"], dc.SEED, 0)
    assert np.array_equal(got, want) and (got == e["unseen"]).all() and dec.all()
    assert (acc == 0).any() and ((acc > 0) & (acc < 8)).any()  # both branches occur (the GPU test relies on it)
    everything = np.full(4, 2, np.int32)
    got, _, _, _, _ = dm.sample(e["P"], e["Q"], None, e["indptr"], e["indices"], everything, 8, dc.SEED, 0)
    assert not got.any()


# ---- 2. properties of the pick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 5, 32])
def test_picks_are_unseen_and_never_the_pad_item(M):
    pr = small(n=300, seed=6, per_user=60)
    got, sc, _, _, acc = dm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], M, 3, 0)
    for u, j in zip(pr["users"], got):
        assert j != 0 and j not in pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]]
    assert (acc == M).all()
    if M > 1:  # the pick's score is the maximum over its candidates: never below the single candidate's
        _, sc1, _, _, _ = dm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], 1, 3, 0)
        assert (sc >= sc1).all() and (sc > sc1).any()


def test_ties_keep_the_earlier_candidate_and_nan_never_wins():
    assert dm.choose(np.array([1.0, 2.0, 2.0, 0.5])) == 1
    assert dm.choose(np.array([np.nan, np.nan])) == 0
    assert dm.choose(np.array([np.nan, -3.0, np.nan, -4.0])) == 1
    assert dm.choose(np.array([0.0, np.nan, 1.0])) == 2
    assert dm.choose(np.array([-0.0, 0.0])) == 0


def test_rank_statistics_of_the_pick():
    """N unseen items with distinct scores, M candidates with replacement: P(rank = r) = ((N-r+1)^M - (N-r)^M) / N^M.
    Chi-square at N = 40, M = 4 over 20,000 draws (cells pooled from the tail until each expects >= 5)."""
    N, M, n, d = 40, 4, 20_000, 8
    I = N + 21
    rng = np.random.default_rng(12)
    P = rng.standard_normal((2, d)).astype(np.float32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    seen_items = np.sort(rng.choice(np.arange(1, I), size=I - 1 - N, replace=False)).astype(np.int32)
    indptr, indices = np.array([0, 0, len(seen_items)], np.int64), seen_items
    unseen = np.array([i for i in range(1, I) if i not in set(seen_items.tolist())])
    s = Q[unseen].astype(np.float64) @ P[1].astype(np.float64)
    assert len(unseen) == N and len(np.unique(s)) == N
    rank_of = np.zeros(I, np.int64)
    rank_of[unseen[np.argsort(-s)]] = np.arange(1, N + 1)
    got, _, _, _, _ = dm.sample(P, Q, None, indptr, indices, np.full(n, 1, np.int32), M, 2024, 0)
    obs = np.bincount(rank_of[got], minlength=N + 1)[1:].astype(np.float64)
    exp = dm.rank_pmf(N, M) * n
    assert abs(dm.rank_pmf(N, M).sum() - 1) < 1e-12 and obs.sum() == n
    k = N
    while exp[k - 1:].sum() < 5:
        k -= 1
    obs, exp = np.append(obs[:k - 1], obs[k - 1:].sum()), np.append(exp[:k - 1], exp[k - 1:].sum())
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    p = dm.chi2_sf(chi2, len(exp) - 1)
    print(f"chi2 {chi2:.2f} over {len(exp)} cells, p = {p:.4g}")
    assert p > 1e-4


def test_the_chi_square_tail_is_the_tabulated_one():
    for x, dof, want in ((3.841, 1, 0.05), (18.307, 10, 0.05), (37.566, 20, 0.01), (59.703, 30, 0.001), (5.0, 30, 1.0)):
        assert abs(dm.chi2_sf(x, dof) - want) < (2e-5 if want < 1 else 1e-4), (x, dof, dm.chi2_sf(x, dof))


# ---- 3. the committed inputs of the GPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", dc.DS)
def test_undecided_share_of_the_gpu_pick_cases(d, bias):
    for M in dc.MS:
        _, _, dec, _, acc = dc.pick_model(M, d, bias)
        share = 1.0 - dec.mean()
        print(f"M {M} d {d} bias {bias}: undecided {share:.4%}")
        assert share <= 0.01 and (acc == M).all()


@pytest.mark.parametrize("d", dc.SEQ_DS)
def test_every_triple_of_the_sequential_cases_is_decided(d):
    check_sequential_case_is_decided(d, dc.SEQ_M)


@pytest.mark.parametrize("d,M", sorted(dc.SEQ_CHUNKED))
def test_every_triple_of_the_chunked_sequential_cases_is_decided(d, M):
    check_sequential_case_is_decided(d, M)


def check_sequential_case_is_decided(d, M):
    P, Q, neg, dec, sc = dc.seq_model(d, M)
    assert dec.all(), int((~dec).sum())
    assert np.isfinite(P).all() and np.isfinite(Q).all() and sc[3] == dc.SEQ_N
    pr = dc.seq_problem(d, M)
    for u, j in zip(pr["users"], neg):
        assert j != 0 and j not in pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]]


def test_the_case_files_cover_every_group_layout_at_a_full_and_a_partial_width():
    """(G, E) and the rows of a chunk as tests/dynamic_cases.py mirrors them from bpr_group_shape.h and
    bpr_scored_plan.h, and what DS, SEQ_DS and SEQ_CHUNKED promise about them."""
    assert [dc.group_shape(d) for d in (1, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [
        (32, 1), (32, 1), (32, 2), (32, 2), (32, 4), (32, 4), (64, 4), (64, 4), (64, 8), (64, 8), (64, 16), (64, 16)]
    assert [dc.inflight_rows(d) for d in (32, 64, 128, 256, 257, 512, 513, 1024)] == [8, 8, 8, 8, 4, 4, 2, 2]
    layouts = {(32, 1), (32, 2), (32, 4), (64, 4), (64, 8), (64, 16)}
    for ds in (dc.DS, dc.SEQ_DS):
        assert {dc.group_shape(d) for d in ds} == layouts
    for G, E in layouts - {(32, 4), (64, 4)}:  # full: every lane's E entries inside the row; partial: some past d
        assert any(dc.group_shape(d) == (G, E) and d == G * E for d in dc.DS)
        assert any(dc.group_shape(d) == (G, E) and d < G * E for d in dc.DS)
    for d, M in dc.SEQ_CHUNKED:
        assert M > dc.inflight_rows(d) == 4
    for d, n in dc.GRID_N.items():
        G = dc.group_shape(d)[0]
        assert dc.GRID_PASS[d] == 2048 * 256 // G < n and n % (64 // G) == 64 // G - 1


@pytest.mark.parametrize("d", sorted(dc.GRID_N))
def test_undecided_share_of_the_gpu_grid_windows(d):
    n = dc.GRID_N[d]
    (lo, hi), (tlo, thi) = dc.grid_windows(d)
    assert lo < dc.GRID_PASS[d] < hi <= n and thi == n and thi - tlo == dc.GRID_WINDOW
    for w in dc.grid_windows(d):
        _, _, dec, _, acc = dc.grid_model(d, w)
        print(f"d {d} draws {w}: undecided {1 - dec.mean():.4%}")
        assert 1.0 - dec.mean() <= 0.01 and (acc == dc.GRID_M).all()


def test_the_twins_of_the_ties_case_fall_into_different_chunks():
    """test_gpu_dynamic's identical-rows case (14 items, 2 seen, M = 8, seed 41) at its wide widths: the accepted lists
    hold both twins 3 and 9 in different chunks of 4 and of 2 rows, in either order, often enough for its assertions."""
    for d in (512, 1024):
        pr = dc.problem(8, 14, d, 2, seed=13, n=1024)
        lists = dm.accepted_lists(pr["indptr"], pr["indices"], 14, pr["users"], 8, 41, 0)
        C = dc.inflight_rows(d)
        cross = [c.index(3) < c.index(9) for c in lists if 3 in c and 9 in c and c.index(3) // C != c.index(9) // C]
        same = [c for c in lists if 3 in c and 9 in c and c.index(3) // C == c.index(9) // C]
        print(f"chunks of {C}: twins in different chunks {len(cross)} (3 first {sum(cross)}), in one chunk {len(same)}")
        assert len(cross) >= 20 and 0 < sum(cross) < len(cross) and same


# ---- 4. the plan ----------------------------------------------------------------------------------------------------------
def test_plan_headers_alone_under_the_host_sanitizers(tmp_path):
    """bpr_scored_plan.h and bpr_stream_plan.h are plain C++: built into a program of its own with
    -fsanitize=address,undefined, tests/dynamic_plan_check.cpp runs clean (the range of M, the grid, no LDS tier for
    dynamic negatives, the uniform and adaptive plans unchanged)."""
    exe = tmp_path / "dynamic_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "dynamic_plan_check.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 5. the C ABI refuses before it touches a device --------------------------------------------------------------------
def test_abi_refusals_need_no_device():
    from revisit_bpr import native

    lib = native.load()
    assert native.NEG_DYNAMIC == 3
    assert lib.bpr_set_dynamic(None, 4) == -1 and b"NULL" in lib.bpr_last_error()
    assert lib.bpr_sample_dynamic(None, None, 0, 4, 0, 0, None, None) == -1
    # the new kind is refused by name (BPR_ERR_UNSUPPORTED = -3) before anything else is looked at
    assert lib.bpr_train_strict(None, None, None, None, 0, 1, 3, 0.5, 0, 0, 0, None) == -3
    assert lib.bpr_train_stream_batched(None, None, None, None, 0, 1, 3, 0.5, 0, 0, 0, None) == -3
    assert lib.bpr_train_stream_acut(None, None, None, None, 1, 3, 0.5, 0, 0, 0, None) == -3
    assert lib.bpr_step(None, None, None, None, 0, native.MODE_STRICT, 3, 0.5, 0, 0, None, None, None) == -3
    assert lib.bpr_fold_in_rows(None, None, 10, 8, None, None, 1, None, 1, 0.1, 0.0, 3, None, None, 0, 0, None,
                                None) == -3
    assert b"dynamic" in lib.bpr_last_error()


def test_schedule_and_trainers_take_the_new_name():
    from revisit_bpr import fast

    u = fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="uniform", hot_lds=0)
    dyn = fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="dynamic")
    assert dyn == u and dyn.hot_lds == 0 and dyn.refresh_lag == 0.0 and dyn.refresh_cus == 0
    with pytest.raises(ValueError, match="LDS tier"):
        fast.resolve_schedule(20109, 128, 10 ** 7, 256, 0.001, sampler="dynamic", hot_lds=64)
    with pytest.raises(ValueError, match="DynamicSampler"):
        fast._refuse_dynamic("dynamic", "StrictTrainer")
    fast._refuse_dynamic("uniform", "StrictTrainer")
