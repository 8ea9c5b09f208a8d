"""The seeded rows of tests/test_gpu_adam_replay.py tell a right Adam replay from a subtly wrong one — shown in float64.

tests/adam_replay_model.py restates the route logic of both lazy replays (`opt_replay_row`, STRICT; `vo_replay`, the
batched stream).  Here, without a GPU:

  * the restatement agrees with exact dense Adam on every seeded row, for every gap k and start s0 the GPU tests use,
    within the suite's own tolerance (test_gpu_parity.close at 2e-5: |err| <= 2e-5 max(1, |w|)) — so a kernel that
    follows its own route logic can meet the oracle;
  * a model with one deliberate error (a series term dropped, the full-tail series for a short gap, the sqrt(v) gate
    removed, the series taken while the bias corrections are still warm, the state decayed by the capped gap) puts at
    least one seeded row outside that tolerance — so the GPU comparison would notice the same error in a kernel;
  * three variations change nothing a float64 comparison can see, and that is asserted too, because it says what the
    constants are: `closed_min` is a cost crossover (the series is exact for every k), the `kk = min(k, kmax)` cap of
    the series only drops terms below 1e-8 of the first, and the twelfth term of the STRICT series is eps-expansion
    head-room (e^11 < 3e-9 at its gate) — dropping down to the batched stream's three terms at the STRICT gate IS seen.
"""
import functools

import numpy as np
import pytest

import adam_replay_model as am

LR, EPS = 0.01, 1e-8
BETAS = [(0.9, 0.999), (0.1, 0.999)]
KS = (2, 3, 15, 16, 17, 175, 176, 177, 400)
TOL = 2e-5


def s0s(betas, deep_warm=True):
    t_sat = am.host_consts(*betas)[1]
    return (t_sat - 200, t_sat - 8, t_sat, 40_000) + ((100, 2000) if deep_warm else ())


def excess(got, want):
    """max of |got - want| / (TOL max(1, |want|)): > 1 means test_gpu_parity.close(got, want, TOL) fails."""
    return float(np.max(np.abs(got - want) / (TOL * np.maximum(1.0, np.abs(want)))))


@functools.lru_cache(maxsize=None)
def table(d, betas):
    w, m, v, cls = am.seeded_rows(96, d, *betas, EPS, seed=d)
    for a in (w, m, v):
        a.setflags(write=False)
    return w, m, v, cls


@functools.lru_cache(maxsize=None)
def dense(d, betas, s0, k):
    w, m, v, _ = table(d, betas)
    return am.dense_zero_steps(w, m, v, s0, k, LR, *betas, EPS)


def model(path, d, betas, s0, k, mutate=(), **over):
    w, m, v, _ = table(d, betas)
    kw = dict(am.path_kw(path, *betas), G=am.lane_geometry(d)[0])
    kw.update(over)
    return am.closed_model(w, m, v, s0, k, LR, *betas, EPS, mutate=mutate, **kw)


def worst(path, betas, mutate=(), **over):
    """The largest excess over the tolerance of (w, m, v) against dense Adam, over the whole sweep."""
    return _worst(path, betas, tuple(mutate), tuple(sorted(over.items())))


@functools.lru_cache(maxsize=None)
def _worst(path, betas, mutate, over):
    over, out = dict(over), 0.0
    for d in (50, 128):
        for s0 in s0s(betas):
            for k in KS:
                got = model(path, d, betas, s0, k, mutate, **over)
                out = max(out, *(excess(g, r) for g, r in zip(got[:3], dense(d, betas, s0, k))))
    return out


def test_host_constants_are_the_documented_ones():
    assert am.host_consts(0.9, 0.999) == (176, 17_321)
    assert am.host_consts(0.1, 0.999) == (9, 17_321)
    assert am.sv_min("batched", 0.9, 0.999, EPS) == pytest.approx(5.46e-7, rel=2e-3)
    assert am.sv_min("strict", 0.9, 0.999, EPS) == pytest.approx(5.46e-8, rel=2e-3)
    assert am.path_kw("batched", 0.9, 0.999)["closed_min"] == 16 and am.path_kw("batched", 0.1, 0.999)["closed_min"] == 3
    assert am.lane_geometry(50) == (32, 2) and am.lane_geometry(128) == (32, 4) and am.lane_geometry(256) == (64, 4)


@pytest.mark.parametrize("d", [50, 128])
@pytest.mark.parametrize("betas", BETAS)
def test_seeded_rows_hold_every_class_in_fp32(d, betas):
    w, m, v, cls = table(d, betas)
    assert w.dtype == m.dtype == v.dtype == np.float32 and (v > 0).all()
    assert not m[cls == am.ZERO_M].any() and m[cls != am.ZERO_M].all() and not w[0].any()
    sv = np.sqrt(v.astype(np.float64))
    ratio = np.abs(m) / sv
    typ = cls == am.TYPICAL
    assert typ.sum() >= 16 and 1e-6 * 0.99 <= v[typ].min() and v[typ].max() <= 1e-3 * 1.01
    assert 0.49 <= ratio[typ].min() and ratio[typ].max() <= 5.01
    gate = cls == am.GATE
    assert gate.sum() == 2 * len(am.GATE_FACTORS) and 1.99 <= ratio[gate].min() and ratio[gate].max() <= 5.01
    for path in am.PATHS:  # rows on both sides of each path's gate, 10 % away from it: fp32 rounding cannot flip them
        f = sv[gate][:, 0] / am.sv_min(path, *betas, EPS)
        for want in am.GATE_FACTORS:
            assert np.isclose(f, want, rtol=1e-3).sum() == 1, (path, want, f)
    for r in np.nonzero(cls == am.MIXED)[0]:
        assert sum((sv[r] < am.sv_min(p, *betas, EPS)).sum() for p in am.PATHS) in (1, 2)  # one element, one or both gates
    assert (cls == am.PADDED).sum() == (4 if d == 50 else 0)


def test_gate_rows_move_by_a_sane_amount():
    """beta1 = 0.9, a 400-step gap: every gate row moves by 0.05 ... 0.5 in float64 (the tables stay sane, and the
    movement is large against the tolerance).  With beta1 = 0.1 the whole tail sums to lr |m| / sqrt(v) / 9."""
    betas = BETAS[0]
    w, _, _, cls = table(128, betas)
    moved = np.abs(dense(128, betas, 40_000, 400)[0] - w)[cls == am.GATE]
    assert 0.05 <= moved.min() and moved.max() <= 0.5, (moved.min(), moved.max())


@pytest.mark.parametrize("k", KS)
def test_three_term_series_truncation_at_the_batched_gate(k):
    """At sqrt(v) = 1.001 sv_min the three-term series is within 1e-5 of the replayed movement (vopt's comment)."""
    betas, s0 = BETAS[0], 40_000
    sv = am.sv_min("batched", *betas, EPS) * 1.001  # (just inside: the gate itself is rounded to fp32)
    w, m, v = np.zeros((1, 1)), np.full((1, 1), 4.0 * sv), np.full((1, 1), sv * sv)
    got = am.closed_model(w, m, v, s0, k, LR, *betas, EPS, **dict(am.path_kw("batched", *betas), closed_min=1))
    want = am.dense_zero_steps(w, m, v, s0, k, LR, *betas, EPS)[0]
    assert got[3].all() and abs(got[0] - want).max() <= 1e-5 * abs(want).max()


@pytest.mark.parametrize("betas", BETAS)
@pytest.mark.parametrize("path", list(am.PATHS))
def test_the_route_logic_of_each_path_meets_dense_adam(path, betas):
    assert worst(path, betas) <= 1.0


@pytest.mark.parametrize("betas", BETAS)
@pytest.mark.parametrize("path", list(am.PATHS))
def test_zero_momentum_rows_do_not_move(path, betas):
    w, _, _, cls = table(50, betas)
    for s0 in s0s(betas):
        got = model(path, 50, betas, s0, 400)[0]
        assert np.array_equal(got[cls == am.ZERO_M], w[cls == am.ZERO_M].astype(np.float64))


# (path, mutation) pairs a float64 comparison cannot see, with the reason in the module docstring
EQUIVALENT = {("strict", "drop_last_term"), ("strict", "series_k_for_kk"), ("batched", "series_k_for_kk"),
              ("strict", "no_closed_min"), ("batched", "no_closed_min")}


@pytest.mark.parametrize("mutation", am.MUTATIONS)
@pytest.mark.parametrize("path", list(am.PATHS))
def test_a_mutated_model_leaves_the_tolerance(path, mutation):
    betas = BETAS[0]
    bad = worst(path, betas, (mutation,))
    if (path, mutation) in EQUIVALENT:
        assert bad <= 1.0 and worst(path, BETAS[1], (mutation,)) <= 1.0
        for d in (50, 128):  # not merely inside the tolerance: the same numbers to a tenth of it (what is left is the
            # three-term truncation at the batched gate, 6e-6 of the movement)
            for s0 in s0s(betas):
                for k in KS:
                    a, b = model(path, d, betas, s0, k, (mutation,)), model(path, d, betas, s0, k)
                    assert np.abs(a[0] - b[0]).max() <= 0.1 * TOL and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    else:
        assert bad > 1.0, (path, mutation, bad)


def test_the_strict_gate_needs_more_than_the_batched_series():
    """The twelfth STRICT term cannot be seen, but the term COUNT can: three terms at the STRICT gate miss."""
    assert worst("strict", BETAS[0], J=3) > 1.0


def test_use_loop_below_gate_false_is_the_gate_mutation():
    for path in am.PATHS:
        assert worst(path, BETAS[0], use_loop_below_gate=False) == worst(path, BETAS[0], ("no_gate",)) > 1.0


@pytest.mark.parametrize("path", list(am.PATHS))
def test_the_lane_rule_sends_a_mixed_rows_lane_to_the_loop(path):
    betas, d = BETAS[0], 50
    _, m, v, cls = table(d, betas)
    closed = model(path, d, betas, 40_000, 400)[3]
    gate = am.sv_min(path, *betas, EPS)
    for r in np.nonzero(cls == am.MIXED)[0]:
        low = np.nonzero(np.sqrt(v[r].astype(np.float64)) < gate)[0]
        if len(low) == 0:  # this row's low element sits under the other path's (higher) gate only
            assert closed[r].all()
            continue
        lane = np.arange(d) % 32 == low[0] % 32
        assert not closed[r, lane].any() and closed[r, ~lane].all()
    pad = cls == am.PADDED
    assert closed[pad].all()
