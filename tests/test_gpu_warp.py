"""The WARP objective on the GPU: the stand-alone kernel (bpr_sample_warp) and k_stream's NEG_WARP branch against the
numpy model (tests/warp_model.py), the uniform sampler (N = 1) and each other.

Violators are compared with the model on DECIDED triples only — those none of whose comparisons, up to the first sure
violator, falls inside the two scores' float32 bounds 2 (d + 1) 2^-24 (sum|p q| + |b|), see tests/warp_model.py — and
every such test first asserts that at most 1 % of its triples are undecided (tests/test_warp_model_cpu.py shows the
same on the CPU).  Between the two kernels, and against the uniform sampler, negatives are compared bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import dynamic_cases as dc
import warp_cases as wc
import warp_model as wm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402

NEG_UNIFORM, NEG_WARP = 1, 4


def engine(pr, bias=True, **kw):
    e = make_engine(pr["P"], pr["Q"], pr["b"] if bias else None, **kw)
    e.bind_seen_csr(dev(pr["indptr"]), dev(pr["indices"]))
    return e


def check_against_model(got, model, what):
    """got = (neg, tries, x_pos, x_neg) numpy arrays of the kernel, model = warp_model.sample's tuple."""
    neg, tries, xp, xn = got
    items, mtries, mxp, mxn, und, eps, _ = model
    print(f"{what}: undecided {und.mean():.4%}, skipped {np.mean(mtries == 0):.3f}, agree {np.mean(neg == items):.4%}")
    assert und.mean() <= 0.01
    dec = ~und
    bad = np.nonzero(dec & ((neg != items) | (tries != mtries)))[0]
    assert bad.size == 0, (what, bad[:5], neg[bad[:5]], items[bad[:5]], tries[bad[:5]], mtries[bad[:5]])
    assert ((neg < 0) == (tries == 0)).all()
    if xp is not None:  # the returned scores stay within the bound (eps = the positive's bound + the largest candidate's)
        assert (np.abs(xp.astype(np.float64) - mxp) <= eps).all(), float(np.abs(xp - mxp).max())
        hit = dec & (items >= 0)
        assert (np.abs(xn.astype(np.float64)[hit] - mxn[hit]) <= eps[hit]).all()
        assert not xn[neg < 0].any()


def gpu_sample(e, pr, N, margin=wc.MARGIN, seed=wc.SEED, offset=0, scores=True):
    out = e.sample_warp(dev(pr["users"]), dev(pr["pos"]), N, seed=seed, offset=offset, margin=margin,
                        return_scores=scores)
    out = [t.cpu().numpy() for t in out]
    return out if scores else out + [None, None]


# ---- 1. violators and tries against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", wc.DS)
def test_violators_tries_and_scores_match_the_model(d, bias):
    pr = wc.pick_problem(d, bias)
    e = engine(pr, bias)
    for N in wc.NS:
        check_against_model(gpu_sample(e, pr, N), wc.pick_model(N, d, bias), f"N {N} d {d} bias {bias}")


def test_bound_item_weights_change_the_candidates_as_the_model_says():
    pr, w, _, _ = wc.weights_problem()
    e = engine(pr, True)
    plain = gpu_sample(e, pr, 10)[0]
    e.bind_item_weights(dev(w))
    for N in (2, 10):
        check_against_model(gpu_sample(e, pr, N), wc.weights_model(N), f"weights N {N}")
    assert (gpu_sample(e, pr, 10)[0] != plain).mean() > 0.3


# ---- 2. every "seen?" structure ---------------------------------------------------------------------------------------------
def fused_negatives(e, pr, N, seed, offset, margin=wc.MARGIN, scalars=None, **kw):
    """The negatives a launch with lr = 0 trains on (-1 = skipped), returned the way the dynamic test obtains them."""
    e.set_optimizer(kind=0, lr=0.0)
    e.set_warp(N, margin)
    negs = torch.full((len(pr["users"]),), -9, dtype=torch.int32, device="cuda")
    e.train_stream(dev(pr["users"]), dev(pr["pos"]), sampler=NEG_WARP, neg=negs, seed=seed, offset=offset,
                   scalars=scalars, **kw)
    return negs


SEEN_STRUCTURES = ["", "csr", "bitmap", "list", "list-overflow", "heavy"]


@pytest.mark.parametrize("seen", SEEN_STRUCTURES)
def test_every_seen_structure_gives_the_stand_alone_negatives(seen, monkeypatch):
    check_seen_structure(seen, 256, monkeypatch)


@pytest.mark.parametrize("seen", SEEN_STRUCTURES)
def test_every_seen_structure_gives_the_stand_alone_negatives_at_sixteen_entries_a_lane(seen, monkeypatch):
    check_seen_structure(seen, 1000, monkeypatch)  # (64, 16), partial: the 10 candidates are five chunks of two rows


def check_seen_structure(seen, d, monkeypatch):
    U, I, n, per_user = 60, 90, 400, 30
    if seen == "list-overflow":  # > 512 seen items per user: the staged list does not hold them
        I, per_user = 1500, 700
    if seen and seen != "heavy":
        monkeypatch.setenv("BPR_SEEN", seen.split("-")[0])
    pr = wc.problem(U, I, d, per_user, seed=5, n=n)
    e = engine(pr, False)
    if seen == "heavy":
        e.set_heavy_users(4, 0)  # more than 4 seen items = heavy: every user's bitmap is staged from the table
    negs = fused_negatives(e, pr, 10, seed=9, offset=100)
    if seen == "heavy":
        assert e.heavy_users()[0] > 0
    want, tries = e.sample_warp(dev(pr["users"]), dev(pr["pos"]), 10, seed=9, offset=100)
    assert torch.equal(negs, want)
    got = negs.cpu().numpy()
    assert (got < 0).any() and (got > 0).any() and (tries.cpu().numpy() > 1).any()
    for u, j in zip(pr["users"], got):
        assert j == -1 or (j != 0 and j not in pr["indices"][pr["indptr"][u]:pr["indptr"][u + 1]])


def test_the_staged_sorted_list_of_a_large_catalogue():
    pr = wc.big_problem()  # I = 70,000, d = 20
    e = engine(pr, False)
    got = gpu_sample(e, pr, 10)
    check_against_model(got, wc.big_model(10), "I 70,000")
    negs = fused_negatives(e, pr, 10, seed=wc.SEED, offset=0)
    assert np.array_equal(negs.cpu().numpy(), got[0])


# (the edge cases at d = 32 keep their names; the same bodies run again at the widths whose chunks are 4 and 2 rows)
def test_users_with_one_unseen_item_with_none_and_with_fewer_than_n():
    check_one_unseen_none_and_fewer_than_n(32)


def test_users_with_one_unseen_item_with_none_and_with_fewer_than_n_at_sixteen_entries_a_lane():
    check_one_unseen_none_and_fewer_than_n(1024)


def check_one_unseen_none_and_fewer_than_n(d):
    ed = wc.one_unseen(d=d)
    e = engine(ed, False)
    neg, tries, _, _ = gpu_sample(e, ed, 8)
    assert (neg == ed["unseen"]).all() and (tries == 1).all()
    n = len(ed["users"])
    nothing = dict(ed, users=np.full(n, 2, np.int32))  # nothing unseen: item 0, as the dynamic sampler
    neg, tries, _, _ = gpu_sample(e, nothing, 8)
    assert not neg.any() and (tries == 1).all()
    few = dict(ed, users=np.full(n, 3, np.int32))      # three unseen items, N = 8
    got = gpu_sample(e, few, 8)
    check_against_model(got, wm.sample(ed["P"], ed["Q"], None, ed["indptr"], ed["indices"], few["users"], few["pos"], 8,
                                       wc.MARGIN, wc.SEED, 0), "three unseen")
    assert np.isin(got[0], (11, 22, 33)).all()
    # the fused kernel walks the same branches
    for case in (ed, nothing, few):
        want = gpu_sample(e, case, 8)[0]
        assert np.array_equal(fused_negatives(e, case, 8, seed=wc.SEED, offset=0).cpu().numpy(), want)


# ---- 3. order: the FIRST violator ------------------------------------------------------------------------------------------
order_problem = wc.order_problem


def test_the_first_violator_wins_not_the_best_and_chunks_past_it_do_not_matter():
    check_first_violator(32)


@pytest.mark.parametrize("d", [512, 1024])
def test_the_first_violator_wins_at_every_place_of_a_chunk_of_four_and_of_two_rows(d):
    assert dc.inflight_rows(d) == (4 if d == 512 else 2)
    check_first_violator(d)


def check_first_violator(d):
    pr = order_problem(d=d)
    e = engine(pr, False)
    lists = wc.order_lists()
    for N in (10, 32):
        model = wm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], N, 1.5, 5, 0,
                          lists=lists)
        assert not model[4].any()
        # the violator at every place k = 1 .. N, and nowhere: every place of every chunk is a stopping point
        assert np.array_equal(np.unique(model[1]), np.arange(N + 1))
        neg, tries, _, _ = gpu_sample(e, pr, N, margin=1.5, seed=5)
        assert np.array_equal(neg, model[0]) and np.array_equal(tries, model[1])
        later_better = [b for b in range(len(neg)) if neg[b] > 0 and max(lists[b][:N]) > neg[b]]
        assert len(later_better) > 20  # first, not best
        if N == 10:
            assert (tries == 9).any()   # the violator sits in the second chunk of eight rows
        else:
            assert (tries == 32).any() and (tries == 0).any()  # the last of 32, and none of 32
        assert np.array_equal(fused_negatives(e, pr, N, seed=5, offset=0, margin=1.5).cpu().numpy(), neg)


def test_a_nan_candidate_never_violates_and_a_nan_positive_skips():
    check_nan_candidate_and_nan_positive(32)


@pytest.mark.parametrize("d", [512, 1024])
def test_a_nan_candidate_never_violates_in_chunks_of_four_and_of_two_rows(d):
    check_nan_candidate_and_nan_positive(d)


def check_nan_candidate_and_nan_positive(d):
    pr = order_problem(n=512, I=12, d=d)
    pr["pos"][:] = 2  # every item but 1 violates at margin 1.5
    pr["Q"][5, 1] = np.nan  # (user 1's factor 1 is zero: 0 * NaN = NaN)
    e = engine(pr, False)
    neg, tries, xp, xn = gpu_sample(e, pr, 8, margin=1.5, seed=41)
    model = wm.sample(pr["P"], pr["Q"], None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], 8, 1.5, 41, 0)
    assert np.array_equal(neg, model[0]) and np.array_equal(tries, model[1])
    assert (neg != 5).all() and (tries > 1).any() and np.isfinite(xn).all()
    pr5 = dict(pr, pos=np.full(512, 5, np.int32))
    neg, tries, xp, _ = gpu_sample(e, pr5, 8, margin=1.5, seed=41)
    assert (neg == -1).all() and not tries.any() and np.isnan(xp).all()
    assert (fused_negatives(e, pr5, 8, seed=41, offset=0, margin=1.5) == -1).all()


# ---- 4. skipped triples write nothing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hot", [False, True])
def test_skipped_triples_write_nothing_and_the_scalars_are_the_models(hot):
    check_skipped_triples(hot, 32)


@pytest.mark.parametrize("hot", [False, True])
def test_skipped_triples_write_nothing_at_sixteen_entries_a_lane(hot):
    check_skipped_triples(hot, 640)  # (64, 16), partial: the 10 candidates are five chunks of two rows


def check_skipped_triples(hot, d):
    pr = wc.skip_problem(d)
    Po, Qo, bo, neg_o, tries_o, und, sco = wc.skip_model(10, d)
    assert not und.any()
    e = engine(pr, True, reg=wc.SEQ_REG)
    if hot:  # the hot block in front of the rows, the skipped users' positive among its items
        e.set_hot_rows(16, 2)
        e.set_hot_items(torch.tensor([pr["top"]] + list(range(1, 16)), dtype=torch.int32))
        assert e.hot_rows() == 16
    e.set_optimizer(kind=0, lr=wc.SEQ_LR)
    e.set_warp(10, wc.MARGIN)
    P0, Q0, b0 = e.P.clone(), e.Q.clone(), e.item_bias.clone()
    negs = torch.full((len(pr["users"]),), -9, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    e.train_stream(dev(pr["users"]), dev(pr["pos"]), sampler=NEG_WARP, neg=negs, seed=3, offset=2 ** 32 - 100,
                   max_inflight=1, scalars=sc)
    got = negs.cpu().numpy()
    assert np.array_equal(got, neg_o), np.nonzero(got != neg_o)[0][:5]
    sk = torch.from_numpy(pr["skipped"]).cuda().long()
    assert (got[np.isin(pr["users"], pr["skipped"])] == -1).all()
    # the skipped users' rows, the item only they touch and its bias: bit-identical
    assert torch.equal(e.P[sk], P0[sk]) and torch.equal(e.Q[pr["top"]], Q0[pr["top"]])
    assert torch.equal(e.item_bias[pr["top"]], b0[pr["top"]])
    # every row no stepped triple touches is bit-identical too (the hot block's deltas folded: nothing in them)
    stepped = got >= 0
    touched = np.zeros(pr["I"], bool)
    touched[pr["pos"][stepped]] = True
    touched[got[stepped]] = True
    quiet = torch.from_numpy(np.nonzero(~touched)[0]).cuda()
    assert torch.equal(e.Q[quiet], Q0[quiet]) and torch.equal(e.item_bias[quiet], b0[quiet])
    # what did step follows the sequential model, and the scalars count the stepped triples only
    s = sc.cpu().numpy().astype(np.float64)
    print(f"hot {hot}: stepped {int(s[3])} of {len(got)}, scalars {s} model {sco}")
    assert s[3] == sco[3] == stepped.sum()
    assert close(s[:3], sco[:3], 1e-5), (s, sco)
    assert close(e.P.cpu().numpy(), Po, 1e-5) and close(e.Q.cpu().numpy(), Qo, 1e-5)
    assert close(e.item_bias.cpu().numpy(), bo, 1e-5)


# ---- 5. the fused kernel on static tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 128, 256, 512, 1000])
def test_fused_negatives_equal_the_stand_alone_kernel_on_static_tables(d):
    pr = wc.pick_problem(d, True)
    e = engine(pr, True, reg=(0.01, 0.02, 0.03))
    P0, Q0, b0 = e.P.clone(), e.Q.clone(), e.item_bias.clone()
    off = 2 ** 32 - 500
    for N in (2, 10, 32):
        sc = torch.zeros(4, device="cuda")
        negs = fused_negatives(e, pr, N, seed=wc.SEED, offset=off, scalars=sc)
        want, _ = e.sample_warp(dev(pr["users"]), dev(pr["pos"]), N, seed=wc.SEED, offset=off)
        assert torch.equal(negs, want)
        assert int(sc[3]) == int((want >= 0).sum()) < len(pr["users"])
    assert torch.equal(e.P, P0) and torch.equal(e.Q, Q0) and torch.equal(e.item_bias, b0)
    # the hot block in front of the rows (bpr_set_hot_rows): the same negatives
    e.set_hot_rows(16, 2)
    e.set_hot_items(torch.arange(1, 17, dtype=torch.int32))
    assert e.hot_rows() == 16
    negs2 = fused_negatives(e, pr, 32, seed=wc.SEED, offset=off)
    assert torch.equal(negs2, want) and torch.equal(e.Q, Q0)


def test_one_try_on_all_violating_users_is_the_uniform_launch():
    pr = wc.pick_problem(32, False)
    P = np.zeros_like(pr["P"])  # zero user rows, no bias, margin > 0: every unseen item violates
    e = engine(dict(pr, P=P), False)
    e.set_optimizer(kind=0, lr=0.0)
    users, pos = dev(pr["users"]), dev(pr["pos"])
    off = 2 ** 32 + 5
    uni = torch.zeros(len(pr["users"]), dtype=torch.int32, device="cuda")
    e.train_stream(users, pos, sampler=NEG_UNIFORM, neg=uni, seed=wc.SEED, offset=off)
    negs = fused_negatives(e, pr, 1, seed=wc.SEED, offset=off)
    assert torch.equal(negs, uni) and torch.equal(negs, e.sample_uniform(users, seed=wc.SEED, offset=off))
    neg, tries = e.sample_warp(users, pos, 1, seed=wc.SEED, offset=off)
    assert torch.equal(neg, uni) and (tries == 1).all()
    # on the scaled rows N = 1 is another draw (the comparison above is not vacuous)
    e2 = engine(pr, False)
    assert (e2.sample_warp(users, pos, 1, seed=wc.SEED, offset=off)[0] != uni).float().mean() > 0.1


# ---- 6. the sequential limit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", wc.SEQ_DS)
def test_sequential_limit_equals_the_sequential_model(d):
    check_sequential_limit(d, wc.SEQ_MAX)


@pytest.mark.parametrize("d,N", sorted(wc.SEQ_CHUNKED))
def test_sequential_limit_with_candidates_over_several_chunks_of_four_rows(d, N):
    assert N > dc.inflight_rows(d) == 4
    check_sequential_limit(d, N)


def check_sequential_limit(d, N):
    pr = wc.seq_problem(d, N)
    Po, Qo, neg_o, tries_o, und, sco = wc.seq_model(d, N)
    assert not und.any()
    e = engine(pr, False, reg=wc.SEQ_REG)
    e.set_optimizer(kind=0, lr=wc.SEQ_LR)
    e.set_warp(N, wc.MARGIN)
    negs = torch.zeros(wc.SEQ_N, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    e.train_stream(dev(pr["users"]), dev(pr["pos"]), sampler=NEG_WARP, neg=negs, seed=9, offset=100,
                   max_inflight=1, scalars=sc)
    got = negs.cpu().numpy()
    assert np.array_equal(got, neg_o), np.nonzero(got != neg_o)[0][:5]
    print(f"d {d} N {N}: skipped {np.mean(got < 0):.3f}, max error P {maxerr(e.P.cpu().numpy(), Po):.3g} "
          f"Q {maxerr(e.Q.cpu().numpy(), Qo):.3g}, scalars {sc.cpu().numpy()} model {sco}")
    assert close(e.P.cpu().numpy(), Po, 1e-5), maxerr(e.P.cpu().numpy(), Po)
    assert close(e.Q.cpu().numpy(), Qo, 1e-5), maxerr(e.Q.cpu().numpy(), Qo)
    assert close(sc.cpu().numpy(), sco, 1e-5)


# ---- 6a. the stand-alone kernel's grid-stride passes and its ragged last wave --------------------------------------------
UNWRITTEN, UNWRITTEN_SCORE = -7, -12345.0


def launch_over_sentinels(e, users, pos, N, offset):
    """bpr_sample_warp into buffers filled with sentinels: (neg, tries, x_pos, x_neg), every element of which was
    written."""
    from revisit_bpr import native

    n = users.numel()
    neg, tries = (torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda") for _ in range(2))
    xp, xn = (torch.full((n,), UNWRITTEN_SCORE, dtype=torch.float32, device="cuda") for _ in range(2))
    e._sync_stream()
    native.check(e._lib.bpr_sample_warp(e._ctx, users.data_ptr(), pos.data_ptr(), n, N, wc.MARGIN, wc.SEED, offset,
                                        neg.data_ptr(), tries.data_ptr(), xp.data_ptr(), xn.data_ptr()))
    assert (neg != UNWRITTEN).all() and (tries != UNWRITTEN).all()
    assert (xp != UNWRITTEN_SCORE).all() and (xn != UNWRITTEN_SCORE).all()
    return neg, tries, xp, xn


@pytest.mark.parametrize("d", sorted(dc.GRID_N))
def test_a_launch_past_the_grid_is_its_slices_and_the_model(d):
    """More draws than one pass of k_sample_scored's grid (dynamic_cases.GRID_N: 8,192 draws a pass at G = 64, 16,384
    at G = 32) with a ragged last wave — at d = 64 an odd tail, the wave's second group without a draw."""
    n, G = dc.GRID_N[d], dc.group_shape(d)[0]
    assert n > dc.GRID_PASS[d] == 2048 * 256 // G and n % (64 // G) == 64 // G - 1 and n % (256 // G) != 0
    pr = wc.grid_problem(d)
    e = engine(pr, True)
    users, pos = dev(pr["users"]), dev(pr["pos"])
    whole = launch_over_sentinels(e, users, pos, wc.GRID_MAX, 0)
    # the whole launch is the launches of its slices, each at its own offset: items, tries and both scores
    for lo in range(0, n, dc.GRID_SLICE):
        hi = lo + dc.GRID_SLICE
        part = e.sample_warp(users[lo:hi], pos[lo:hi], wc.GRID_MAX, seed=wc.SEED, offset=lo, margin=wc.MARGIN,
                             return_scores=True)
        for a, b in zip(whole, part):
            assert torch.equal(a[lo:hi], b), lo
    # and the model's draws across the pass boundary and at the tail
    got = [t.cpu().numpy() for t in whole]
    for lo, hi in dc.grid_windows(d):
        check_against_model([a[lo:hi] for a in got], wc.grid_model(d, (lo, hi)), f"d {d} draws {lo} .. {hi}")


def test_a_zero_weight_takes_only_its_l2_step():
    ed = wc.one_unseen()  # n_unseen = 1: L = log(max(1, 1 // tries)) = 0 for every stepped triple
    n = 16
    pr = dict(ed, users=ed["users"][:n], pos=ed["pos"][:n])
    e = engine(pr, False, reg=wc.SEQ_REG)
    e.set_optimizer(kind=0, lr=wc.SEQ_LR)
    e.set_warp(8, wc.MARGIN)
    P, Q = pr["P"].copy(), pr["Q"].copy()
    neg_o, tries_o, und, sco = wm.train_sequential(P, Q, None, pr["indptr"], pr["indices"], pr["users"], pr["pos"], 8,
                                                   wc.MARGIN, wc.SEQ_LR, wc.SEQ_REG, seed=wc.SEED, offset=0)
    assert not und.any() and (neg_o == ed["unseen"]).all() and sco[0] == 0.0 and sco[1] > 0
    negs = torch.zeros(n, dtype=torch.int32, device="cuda")
    sc = torch.zeros(4, device="cuda")
    e.train_stream(dev(pr["users"]), dev(pr["pos"]), sampler=NEG_WARP, neg=negs, seed=wc.SEED, offset=0,
                   max_inflight=1, scalars=sc)
    assert np.array_equal(negs.cpu().numpy(), neg_o)
    s = sc.cpu().numpy()
    assert s[0] == 0.0 and s[3] == n and close(s[1:3], sco[1:3], 1e-5)
    # the user row only shrinks: P[1] (1 - lr alpha_user)^n, no gradient of the loss in it
    want = pr["P"][1].astype(np.float64) * (1 - wc.SEQ_LR * wc.SEQ_REG[0]) ** n
    assert close(e.P[1].cpu().numpy(), want, 1e-5) and close(e.P.cpu().numpy(), P, 1e-5)
    assert close(e.Q.cpu().numpy(), Q, 1e-5) and not np.array_equal(Q[ed["unseen"]], pr["Q"][ed["unseen"]])


# ---- 7. the Python surface --------------------------------------------------------------------------------------------------
def small_model(d=32, U=200, I=120, seed=3):
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    data = synthetic.generate_structured(U, I, 4000, seed=seed)
    torch.manual_seed(seed)
    model = BPR(fuse_forward=True,
                logits_model=MF(torch.nn.Embedding(data.num_users, d, padding_idx=0),
                                torch.nn.Embedding(data.num_items, d, padding_idx=0)),
                reg_alphas={"user": 0.0016, "item": 0.0001, "neg": 0.00375}).cuda()
    t = {k: torch.from_numpy(getattr(data, k)).cuda() for k in ("users", "items", "indptr", "indices")}
    return data, model, t


def test_engine_set_warp_and_sample_warp():
    from revisit_bpr import native

    pr = wc.pick_problem(32, True)
    e = engine(pr, True)
    users, pos = dev(pr["users"]), dev(pr["pos"])
    neg, tries = e.sample_warp(users, pos, 10, seed=1)
    neg2, tries2, xp, xn = e.sample_warp(users.long(), pos.long(), 10, seed=1, return_scores=True)
    assert torch.equal(neg, neg2) and torch.equal(tries, tries2) and neg.dtype == tries.dtype == torch.int32
    assert xp.dtype == xn.dtype == torch.float32 and ((neg < 0) == (tries == 0)).all()
    hit = neg >= 0
    assert (xn[hit] > xp[hit] - 1.0).all() and (tries[hit] >= 1).all() and (tries <= 10).all()
    wide = e.sample_warp(users, pos, 10, seed=1, margin=1e6)[1]
    assert (wide == 1).all()  # everything violates a huge margin
    e.set_warp(32, 0.5)
    for bad in ((0, 1.0), (33, 1.0), (10, 0.0), (10, -1.0), (10, math.inf), (10, math.nan)):
        with pytest.raises(native.BprError):
            e.set_warp(*bad)
        with pytest.raises(native.BprError):
            e.sample_warp(users, pos, bad[0], seed=1, margin=bad[1])
    with pytest.raises(ValueError):
        e.sample_warp(users, pos[:-1], 10, seed=1)


def test_stream_trainer_trains_an_epoch_of_warp_scheduled_as_uniform():
    from revisit_bpr import fast

    data, model, t = small_model()
    tr = fast.StreamTrainer(model, t["users"], t["items"], t["indptr"], t["indices"], lr=0.05, sampler="warp",
                            max_sampled=10, margin=1.0, seed=5)
    uni = fast.resolve_schedule(tr.engine.I, tr.engine.d, data.nnz, 256, 0.05, sampler="uniform", refresh_lag=0.0,
                                refresh_cus=0, hot_lds=0)
    assert tr.schedule == uni and tr.schedule.hot_lds == 0 and tr.schedule.refresh_lag == 0.0
    before = model.logits_model.get_features()["user"].data.clone()
    first = tr.train_epoch()
    second = tr.train_epoch()
    assert 0 < first["triples"] <= data.nnz and 0 < second["triples"] <= data.nnz
    assert np.isfinite(second["loss"]) and second["bpr_loss"] > 0
    assert not torch.equal(model.logits_model.get_features()["user"].data, before)
    assert tr.engine.refresh_info()["route"] is None and not tr.engine.refresh_pending()
    assert tr.engine.lds_launches == 0
    for cls, args in ((fast.StrictTrainer, (model, torch.optim.SGD(model.parameters(), lr=0.05))),
                      (fast.BatchedStreamTrainer, (model, torch.optim.SGD(model.parameters(), lr=0.05)))):
        with pytest.raises(ValueError, match="plain-SGD STREAM kernel only"):
            cls(*args, t["users"], t["items"], t["indptr"], t["indices"], sampler="warp")


def test_example_cli_runs_with_the_warp_objective(tmp_path, caplog):
    import importlib.util
    import logging
    from pathlib import Path

    from click.testing import CliRunner

    from revisit_bpr.datasets import interactions, synthetic

    data = synthetic.generate_structured(800, 300, 20000, seed=3, eval_users=800)
    interactions.write_dataset(data, tmp_path)
    spec = importlib.util.spec_from_file_location(
        "bpr_example", Path(__file__).resolve().parents[1] / "revisit-bpr_amd" / "example.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with caplog.at_level(logging.INFO, logger="example"):
        res = CliRunner().invoke(mod.main, [str(tmp_path), "--num-users", str(data.num_users), "--num-items",
                                            str(data.num_items), "--embedding-dim", "32", "--epochs", "1", "--lr",
                                            "0.05", "--sampler", "warp", "--max-sampled", "10", "--margin", "1.0"],
                                 catch_exceptions=False, standalone_mode=False)
    assert res.exit_code == 0, res.output
    nd = [float(r.getMessage().split("|")[1]) for r in caplog.records if r.getMessage().startswith("ndcg@100")]
    assert len(nd) == 1 and math.isfinite(nd[0]) and 0.0 < nd[0] <= 1.0, nd


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from revisit_bpr import native

    pr = wc.problem(16, 40, 32, 5, seed=1, n=64)
    e = engine(pr, False)
    e.set_optimizer(kind=0, lr=0.05)
    lib, ctx = e._lib, e._ctx
    users, pos = dev(pr["users"]), dev(pr["pos"])
    out = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    tries = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    P0, Q0 = e.P.clone(), e.Q.clone()
    INVALID, UNSUPPORTED = -1, -3
    f = ctypes.c_float
    for N, m in ((0, 1.0), (33, 1.0), (-1, 1.0), (10, 0.0), (10, -2.0), (10, math.inf), (10, math.nan)):
        assert lib.bpr_sample_warp(ctx, users.data_ptr(), pos.data_ptr(), 64, N, f(m), 1, 0, out.data_ptr(),
                                   tries.data_ptr(), None, None) == INVALID
        assert lib.bpr_set_warp(ctx, N, f(m)) == INVALID
    for args in ((None, pos.data_ptr(), out.data_ptr(), tries.data_ptr()),
                 (users.data_ptr(), None, out.data_ptr(), tries.data_ptr()),
                 (users.data_ptr(), pos.data_ptr(), None, tries.data_ptr()),
                 (users.data_ptr(), pos.data_ptr(), out.data_ptr(), None)):
        assert lib.bpr_sample_warp(ctx, args[0], args[1], 64, 10, f(1.0), 1, 0, args[2], args[3], None, None) == INVALID

    def warp_named():
        return b"WARP" in lib.bpr_last_error()

    assert lib.bpr_train_strict(ctx, users.data_ptr(), pos.data_ptr(), out.data_ptr(), 64, 32, NEG_WARP, f(0.1), 1, 0,
                                0, None) == UNSUPPORTED and warp_named()
    assert lib.bpr_train_stream_batched(ctx, users.data_ptr(), pos.data_ptr(), out.data_ptr(), 64, 32, NEG_WARP,
                                        f(0.1), 1, 0, 0, None) == UNSUPPORTED and warp_named()
    assert lib.bpr_train_stream_acut(ctx, users.data_ptr(), pos.data_ptr(), out.data_ptr(), 64, NEG_WARP, f(0.1), 1,
                                     0, 0, None) == UNSUPPORTED and warp_named()
    assert lib.bpr_step(ctx, users.data_ptr(), pos.data_ptr(), out.data_ptr(), 64, native.MODE_STRICT, NEG_WARP,
                        f(0.1), 1, 0, None, None, None) == UNSUPPORTED and warp_named()
    indptr = dev(np.array([0, 3], np.int64))
    items = dev(np.array([1, 2, 3], np.int32))
    pnew = torch.zeros(1, 32, device="cuda")
    assert lib.bpr_fold_in_rows(e.Q.data_ptr(), None, 40, 32, indptr.data_ptr(), items.data_ptr(), 1, None, 1,
                                f(0.1), f(0.0), NEG_WARP, None, None, 1, 0, pnew.data_ptr(), None) == UNSUPPORTED
    assert warp_named()
    assert lib.bpr_fold_in_item_rows(e.P.data_ptr(), 16, e.Q.data_ptr(), None, 40, 32, None, None, indptr.data_ptr(),
                                     items.data_ptr(), 1, None, 1, f(0.1), f(0.0), NEG_WARP, None, None, 1, 0,
                                     pnew.data_ptr(), None, None) == UNSUPPORTED and warp_named()
    torch.cuda.synchronize()
    assert (out == -7).all() and (tries == -7).all() and not pnew.any()
    assert torch.equal(e.P, P0) and torch.equal(e.Q, Q0)
    # and the kind is accepted where the header says so: bpr_train_stream, _cut and STREAM-mode bpr_step
    e.set_warp(32, 1.0)
    e.train_stream(users, pos, sampler=NEG_WARP, neg=out, seed=1)
    assert (out != -7).all() and (out > 0).any()
    out.fill_(-7)
    e.train_stream(users, pos, sampler=NEG_WARP, neg=out, seed=1, cut=True)
    assert (out != -7).all()
    out.fill_(-7)
    assert lib.bpr_step(ctx, users.data_ptr(), pos.data_ptr(), out.data_ptr(), 64, native.MODE_STREAM, NEG_WARP,
                        f(0.1), 1, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert (out != -7).all()
