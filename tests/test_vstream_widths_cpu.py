"""The cases of tests/test_gpu_vstream_widths.py (vstream_scored_model.WIDTHS and the three WIDTH_*_CASES tables), shown
fit for purpose before a GPU sees them: the tables cover what they claim, the caps cannot bite a correct kernel, the
things the GPU file asserts do occur, every case moves the last column of a row, and two deliberately wrong models — a
dropped tail, a view one step off — fail the very assertions the GPU file makes.  No GPU."""
import numpy as np
import pytest

import opt_replay_model as orm
import vstream_scored_model as vm
from test_gpu_vstream_scored import agree  # plain numpy: the check the GPU file applies

U, I, N, REG, TOL = vm.U, vm.I, vm.N, vm.REG, vm.TOL
OFFSET = 1000
LAYOUTS = [(32, 1), (32, 2), (32, 4), (64, 4), (64, 8), (64, 16)]
ident = lambda c: "-".join(str(x) for x in c)  # noqa: E731


def _problem(d, bias, seed):
    P, Q, b, indptr, indices = vm.problem(U, I, d, bias, seed, vm.SCALE)
    users, pos = vm.triples(indptr, indices, N, seed + 100)
    return P, Q, b, indptr, indices, users, pos


def _run(pr, case_opt, kind, K, B, seed, n=N, **kw):
    P, Q, b, indptr, indices, users, pos = pr
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    d = P.shape[1]
    res = vm.run(Pm, Qm, bm, indptr, indices, users[:n], pos[:n], B, kind, K, vm.warp_margin(d), vm.OPTS[case_opt], REG,
                 seed=seed, offset=OFFSET, tol=TOL, **kw)
    return Pm, Qm, bm, res


def _last_column_moves(pr, Pm, Qm, res):
    """Over the rows a stepped triple touches, the last column of both tables moves by more than 50 * TOL."""
    d = pr[0].shape[1]
    for name, new, old, rows in (("P", Pm, pr[0], res["rows"][0]), ("Q", Qm, pr[1], res["rows"][1])):
        rows = sorted(rows)
        moved = np.abs(new[rows, d - 1].astype(np.float64) - old[rows, d - 1])
        print(f"{name}[:, {d - 1}]: max move {moved.max():.3g} over {len(rows)} touched rows")
        assert moved.max() > 50 * TOL, name


# ---- the tables say what they claim ---------------------------------------------------------------------------------------
def test_the_layout_helper_is_the_strict_files_rule():
    for d in range(1, 1025):
        assert vm.layout(d) == orm.layout(d), d
    for G, E in LAYOUTS:
        ds = [d for d in range(1, 1025) if vm.layout(d) == (G, E)]
        have = [d for d in vm.WIDTHS if d in ds]
        # the smallest, the largest and a ragged width; the layouts no other file runs have all three here, the
        # others may count the 8, 32, 128 and 256 of tests/test_gpu_vstream_scored.py for the largest
        other = [] if (G, E) in ((64, 8), (64, 16)) else [32, 128, 256]
        assert min(ds) in have and max(ds) in have + other and any(d % G for d in have), (G, E)
    assert vm.tail_start(1024) == 960 and vm.tail_start(512) == 448 and vm.tail_start(64) == 32
    assert vm.tail_start(257) == 256 and vm.tail_start(33) == 32 and vm.tail_start(1000) == 960 and vm.tail_start(20) == 0


def test_the_step_cases_cover_every_width_kind_optimizer_and_axis_value():
    cases = vm.WIDTH_STEP_CASES
    assert 36 <= len(cases) <= 44 and len(set(cases)) == len(cases)
    for d in vm.WIDTHS:
        assert {c[3] for c in cases if c[0] == d} == {vm.DYNAMIC, vm.WARP}, d
        if d >= 257:
            assert {c[2] for c in cases if c[0] == d} == set(vm.OPTS), d
    for G, E in ((64, 8), (64, 16)):
        mine = [c for c in cases if vm.layout(c[0]) == (G, E)]
        for opt in vm.OPTS:
            assert {c[1] for c in mine if c[2] == opt} == {False, True}, (G, E, opt)
    assert {c[1] for c in cases} == {False, True} and {c[6] for c in cases} == {-1, 0, 1}
    assert {c[5] for c in cases} == {1, 4, 32}
    assert {c[4] for c in cases if c[3] == vm.DYNAMIC} == {1, 4, 32}
    assert {c[4] for c in cases if c[3] == vm.WARP} == {1, 10, 32}
    spill = {(c[2], c[1]) for c in cases if vm.layout(c[0]) == (32, 4)}
    assert ("adam_09", True) in spill and ("rmsprop", True) in spill  # the E = 4 kernels that spill
    assert all(c[6] == -1 for c in cases if c[5] < 16)  # (vs_direct acts from B = 16 on)


def test_the_pick_and_full_cases_cover_the_layouts():
    for G, E in LAYOUTS[1:]:
        assert {c[3] for c in vm.WIDTH_PICK_CASES if vm.layout(c[0]) == (G, E)}, (G, E)
    assert {c[2] for c in vm.WIDTH_PICK_CASES} == set(vm.OPTS)
    assert {c[3] for c in vm.WIDTH_PICK_CASES if c[0] >= 257} == {vm.DYNAMIC, vm.WARP}
    full = vm.WIDTH_FULL_CASES
    assert {c[0] for c in full} >= {64, 257, 512, 513, 1024}
    for G, E in LAYOUTS:
        assert {c[3] for c in full if vm.layout(c[0]) == (G, E)} >= {vm.DYNAMIC, vm.WARP}, (G, E)
    for G, E in ((64, 8), (64, 16)):
        mine = [c for c in full if vm.layout(c[0]) == (G, E)]
        assert {c[2] for c in mine} == set(vm.OPTS) and {c[1] for c in mine} == {False, True}
        assert vm.UNIFORM in {c[3] for c in mine}
    assert len({c[5] for c in full}) == len(full)


# ---- the pick cases ---------------------------------------------------------------------------------------------------------
def _view_one_step_off(pr, case, res):
    """The mutant "candidates scored on the post-step tables": batch by batch the model takes its step (on the picks
    of the true run), and the batch is drawn on what the step left."""
    d, bias, opt, kind, K, B, seed = case
    P, Q, b, indptr, indices, users, pos = pr
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    neg, tries, st = np.zeros(N, np.int32), np.zeros(N, np.int32), None
    for k, lo in enumerate(range(0, N, B)):
        sl = slice(lo, min(lo + B, N))
        args = (indptr, indices, users[sl], pos[sl], B, kind, K, vm.warp_margin(d), vm.OPTS[opt], REG)
        st = vm.run(Pm, Qm, bm, *args, seed=seed, offset=OFFSET + lo, t0=k, state=st,
                    given=(res["neg"][sl], res["tries"][sl]))["state"]
        late = vm.run(Pm.copy(), Qm.copy(), None if bm is None else bm.copy(), *args, seed=seed, offset=OFFSET + lo,
                      t0=k + 1, state={n: v.copy() for n, v in st.items()})
        neg[sl], tries[sl] = late["neg"], late["tries"]
    return neg, tries


@pytest.mark.parametrize("case", vm.WIDTH_PICK_CASES, ids=ident)
def test_pick_cases_keep_the_cap_slack_and_tell_a_stale_view(case):
    d, bias, opt, kind, K, B, seed = case
    pr = _problem(d, bias, seed)
    Pm, Qm, bm, res = _run(pr, opt, kind, K, B, seed, also=np.float32)
    differ, unexcused = vm.excused(res["neg_also"], res["tries_also"], res)
    inside = int((res["gap"] < res["bound"]).sum())
    print(f"{case}: fp32 scoring differs on {differ}, {unexcused} outside the bound; {inside} of {N} inside the bound")
    assert unexcused == 0 and differ <= vm.CAP * N
    assert inside <= vm.CAP * N  # the cap holds even if EVERY triple inside the bound were to disagree
    if kind == vm.WARP:
        assert (res["neg"] < 0).any() and (res["tries"] > 1).any() and (res["tries"] == 1).any()
    assert len(set(res["neg"][B:].tolist())) > 10  # the later batches do draw (the GPU file asserts it)
    _last_column_moves(pr, Pm, Qm, res)
    neg, tries = _view_one_step_off(pr, case, res)
    differ, unexcused = vm.excused(neg[B:], tries[B:], {k: res[k][B:] for k in ("neg", "tries", "gap", "bound")})
    print(f"{case}: a view one step off changes {differ} later-batch picks, {unexcused} of them outside the bound")
    assert unexcused >= 1  # the GPU file's `unexcused == 0` fails


# ---- the step cases -------------------------------------------------------------------------------------------------------
_step_runs = {}


def _step_run(case):
    if case not in _step_runs:
        d, bias, opt, kind, K, B, _ = case
        pr = _problem(d, bias, vm.STEP_SEED)
        _step_runs[case] = (pr,) + _run(pr, opt, kind, K, B, 7)
    return _step_runs[case]


@pytest.mark.parametrize("case", vm.WIDTH_STEP_CASES, ids=ident)
def test_step_cases_skip_wait_and_move_the_last_column(case):
    d, bias, opt, kind, K, B, _ = case
    pr, Pm, Qm, bm, res = _step_run(case)
    if kind == vm.WARP:
        print(f"{case}: {(res['neg'] < 0).sum()} skipped, {(res['tries'] > 1).sum()} with tries > 1")
        assert (res["neg"] < 0).any()
        assert K == 1 or (res["tries"] > 1).any()  # (one try cannot be late)
    _last_column_moves(pr, Pm, Qm, res)
    assert np.abs(Pm - pr[0]).max() > 1e-3 and np.abs(Qm - pr[1]).max() > 1e-3  # (the GPU file asserts it)


@pytest.mark.parametrize("case", vm.WIDTH_STEP_CASES, ids=ident)
def test_a_dropped_tail_fails_the_step_cases_check(case, monkeypatch):
    """The mutant "the row's last element slot never reaches the step": the gradient's columns from
    vstream_scored_model.tail_start(d) on are zeroed before the optimizer step.  Its tables, fed the true run's picks as
    the GPU file feeds the model the device's, fail `agree` in P and in Q — at every width, E = 1 (where the slot is the
    whole row) included."""
    d, bias, opt, kind, K, B, _ = case
    pr, Pm, Qm, bm, res = _step_run(case)
    true_grad, cut = vm.batch_grad, vm.tail_start(d)

    def dropped(*a, **kw):
        out = true_grad(*a, **kw)
        out[0][:, cut:] = 0
        out[1][:, cut:] = 0
        return out

    monkeypatch.setattr(vm, "batch_grad", dropped)
    Px, Qx, bx, _ = _run(pr, opt, kind, K, B, 7, given=(res["neg"], res["tries"]))
    cfg = vm.OPTS[opt]
    assert not agree(Px, Pm, cfg) and not agree(Qx, Qm, cfg)


# ---- the one-batch cases of the 256-thread block ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", vm.WIDTH_FULL_CASES, ids=ident)
def test_full_cases_one_step_moves_the_last_column(case):
    d, bias, opt, sampler, K, seed = case
    pr = _problem(d, bias, seed)
    P, Q, b, indptr, indices, users, pos = pr
    if sampler == vm.UNIFORM:
        Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
        negs, _ = vm.uniform_loop(Pm, Qm, bm, indptr, indices, users, pos, N, vm.OPTS[opt], REG, seed, OFFSET)
        res = {"rows": [set(users.tolist()) - {0}, set(pos.tolist()) | set(negs.tolist())]}
    else:
        Pm, Qm, bm, res = _run(pr, opt, sampler, K, N, seed)
        assert res["steps"] == 1
        if sampler == vm.WARP:
            assert (res["neg"] < 0).any() and (K == 1 or (res["tries"] > 1).any())
    _last_column_moves(pr, Pm, Qm, res)
