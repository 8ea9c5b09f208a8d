"""The seeded tables of tests/test_gpu_opt_replay.py tell a right lazy replay from a subtly wrong one, at every register
layout of the STRICT kernels — shown without a GPU.

  * tests/opt_replay_model.py's DIMS put each of the six (G, E) layouts at two dims at least, one with a partial last
    element;
  * `replay_float64`, a step-by-step float64 loop, agrees with the dense oracle (`oracle.step`, pinned to torch.optim by
    tests/golden/) on every row a batch does not touch, for every kind, dim and gap the GPU tests use, within the
    tolerances the GPU tests apply — so the model stands for the oracle, not for the kernel;
  * every mutant of that loop (the gap off by one, a feature at the edge of a layout left out, a lost factor, the bias
    left out) differs from it by ten times the tolerance the GPU test applies to a quantity it compares (weights, state,
    or the logits of the touching batch), so fp32 rounding cannot hide the same defect in a kernel.

`tables`, `touch_batch_with_pads` and `reference` are shared with the GPU file.
"""
import functools

import numpy as np
import pytest

import opt_replay_model as om
import oracle
from test_gpu_adam_replay import B1, BUSY, busy_steps, rel_state_ok, touch_batch
from test_gpu_parity import close

REG = (0.0016, 0.0001, 0.00375)  # test_gpu_vstream.REG
TOL, STATE_REL = 2e-5, 1e-4  # test_gpu_parity.close's tol; rel_state_ok's relative bound
S0 = 1000
ROWS = om.ROWS
STATE = ("mP", "vP", "mQ", "vQ", "mb", "vb")
QUIET = np.ones(ROWS, bool)
QUIET[list(BUSY)] = False


@functools.lru_cache(maxsize=None)
def tables(kind, d):
    """(user table, item table with the bias) as opt_replay_model.seeded_state gives them, read-only."""
    sP, sQ = om.seeded_state(kind, ROWS, d, seed=d), om.seeded_state(kind, ROWS, d, seed=d + 1000)
    for s in (sP, sQ):
        for a in s.values():
            if a is not None:
                a.setflags(write=False)
    return sP, sQ


def as_engine(sP, sQ):
    """The seeded tables under the names the engine and the oracle use."""
    return dict(P=sP["w"], Q=sQ["w"], b=sQ["b"], mP=sP["m"], vP=sP["v"], mQ=sQ["m"], vQ=sQ["v"], mb=sQ["mb"], vb=sQ["vb"])


def touch_batch_with_pads():
    """test_gpu_adam_replay.touch_batch (every row but the pad row once as user, positive, negative) and three more
    triples: the pad user; the pad item as the positive; the pad item as the negative."""
    u, p, j = touch_batch()
    return (np.concatenate([u, [0, 11, 12]]).astype(np.int32), np.concatenate([p, [21, 0, 22]]).astype(np.int32),
            np.concatenate([j, [31, 32, 0]]).astype(np.int32))


def oracle_opt(kind_or_cfg):
    cfg = om.KINDS[kind_or_cfg] if isinstance(kind_or_cfg, str) else kind_or_cfg
    return oracle.make_opt(cfg["kind"], **{n: x for n, x in cfg.items() if n != "kind"})


def dense_reference(seeded, opt, s0, k):
    """The dense oracle from a seeded state (names as `as_engine`): read-only dicts after the k busy steps and after the
    touching batch, the latter with its logits under "lp", "ln"."""
    cur = {n: (None if a is None else np.array(a, np.float32)) for n, a in seeded.items()}
    st = {n: cur[n] for n in STATE if cur[n] is not None}
    u, p, j = busy_steps(k)
    for t in range(k):
        sl = slice(t * B1, (t + 1) * B1)
        oracle.step(cur["P"], cur["Q"], cur["b"], u[sl], p[sl], j[sl], opt, s0 + t + 1, st, REG)
    flushed = {n: (None if a is None else a.copy()) for n, a in cur.items()}
    lp, ln, _ = oracle.step(cur["P"], cur["Q"], cur["b"], *touch_batch_with_pads(), opt, s0 + k + 1, st, REG,
                            pad_user=0, pad_item=0)  # the pads Engine binds by default
    cur.update(lp=lp, ln=ln)
    for r in (flushed, cur):
        for a in r.values():
            if a is not None:
                a.setflags(write=False)
    return flushed, cur


@functools.lru_cache(maxsize=None)
def reference(kind, d, k):
    return dense_reference(as_engine(*tables(kind, d)), oracle_opt(kind), S0, k)


def model_logits(rP, rQ):
    """Logits of the touching batch from replayed tables (dicts of opt_replay_model.replay_tables), in float64."""
    u, p, j = touch_batch_with_pads()
    return ((rP["w"][u] * rQ["w"][p]).sum(1) + rQ["b"][p], (rP["w"][u] * rQ["w"][j]).sum(1) + rQ["b"][j])


def test_every_layout_is_held_twice_and_once_with_a_partial_last_element():
    assert om.DIMS == [1, 32, 33, 64, 65, 100, 129, 256, 257, 300, 512, 513, 1000, 1024]
    by = {}
    for d in om.DIMS:
        by.setdefault(om.layout(d), []).append(d)
    assert sorted(by) == [(32, 1), (32, 2), (32, 4), (64, 4), (64, 8), (64, 16)]
    for (G, E), ds in by.items():
        assert len(ds) >= 2 and any(d % G for d in ds), (G, E, ds)
        assert min(ds) == (1 if E == 1 else 129 if (G, E) == (64, 4) else G * E // 2 + 1), (G, E, ds)  # its smallest d
        assert max(ds) == G * E or (G, E) == (32, 4), (G, E, ds)  # its largest (d = 128 is test_gpu_parity's own dim)
    assert [d for d in range(1, 1025) if om.layout(d) != om.layout(d - 1 or 1)] == [33, 65, 129, 257, 513]
    # d = 300: lanes 44 ... 63 hold four live elements and one padding element of the five slots in use
    G, E = om.layout(300)
    assert (G, E) == (64, 8) and [sum(e * G + gl < 300 for e in range(E)) for gl in (43, 44, 63)] == [5, 4, 4]


@pytest.mark.parametrize("kind", list(om.KINDS))
def test_seeded_state_is_fp32_with_still_rows_and_a_zero_pad_row(kind):
    for d in om.DIMS:
        sP, sQ = tables(kind, d)
        for s in (sP, sQ):
            assert s["w"].dtype == np.float32 and s["w"].shape == (ROWS, d) and not s["w"][0].any()
            assert (s["m"] is not None) == om.has_m(kind) and (s["v"] is not None) == om.has_v(kind)
            if s["m"] is not None:
                assert not s["m"][s["still"]].any() and s["m"][~s["still"]].all()
                assert not s["mb"][s["still_b"]].any() and s["mb"][~s["still_b"]].all() and s["mb"][0] != 0
            if s["v"] is not None:
                assert not s["v"][0].any() and (s["v"][1:] > 0).all() and (s["vb"] > 0).all()
            assert not s["still"][list(BUSY)].any()
        assert not np.array_equal(sP["w"], sQ["w"])


@pytest.mark.parametrize("k", om.GAPS)
@pytest.mark.parametrize("kind", list(om.KINDS))
def test_the_float64_loop_is_the_dense_oracle_on_untouched_rows(kind, k):
    for d in om.DIMS:
        sP, sQ = tables(kind, d)
        want, _ = reference(kind, d, k)
        rP, rQ = om.replay_tables(kind, sP, k), om.replay_tables(kind, sQ, k)
        got = as_engine(rP, rQ)
        for n in ("P", "Q", "b"):
            assert close(got[n][QUIET], want[n][QUIET], TOL), (d, n)
        for n in STATE:
            assert (got[n] is None) == (want[n] is None), (d, n)
            if got[n] is not None:
                assert close(got[n][QUIET], want[n][QUIET], TOL) and rel_state_ok(got[n][QUIET], want[n][QUIET]), (d, n)
        for s, r in ((sP, rP), (sQ, rQ)):  # m = 0: not moved at all; plain RMSprop moves no row
            frozen = s["still"] if om.has_m(kind) else np.ones(ROWS, bool)
            assert np.array_equal(r["w"][frozen], s["w"][frozen].astype(np.float64))


def excess(got, want, rel=None):
    """max |got - want| over the GPU test's allowance for the quantity: > 1 fails that test, >= 10 fails it with fp32
    rounding (1e-7 relative per operation, a few hundred operations) nowhere near bridging the difference.  State is held
    by `close` AND by rel_state_ok: missing either fails."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    out = float(np.max(err / (TOL * np.maximum(1.0, np.abs(want)))))
    if rel is not None:
        out = max(out, float(np.max(err / (rel * np.abs(want) + 1e-30))))
    return out


@functools.lru_cache(maxsize=None)
def mutant_excess(name, kind, d, k):
    """dict quantity -> excess of the mutant against replay_float64 on the quiet rows / the touching batch's logits."""
    run = om.MUTANTS[name][2]
    sP, sQ = tables(kind, d)
    good = (om.replay_tables(kind, sP, k), om.replay_tables(kind, sQ, k))
    bad = (run(kind, sP, k), run(kind, sQ, k))
    g, b = as_engine(*good), as_engine(*bad)
    out = dict(weights=max(excess(b[n][QUIET], g[n][QUIET]) for n in ("P", "Q", "b")),
               state=max(excess(b[n][QUIET], g[n][QUIET], STATE_REL) for n in STATE if g[n] is not None),
               logits=max(excess(x, y) for x, y in zip(model_logits(*bad), model_logits(*good))))
    return out


def cases_of(name):
    kinds, dims_ok, _ = om.MUTANTS[name]
    return [(kind, d, k) for kind in kinds for d in om.DIMS if dims_ok(d) for k in om.GAPS]


def test_the_mutants_are_the_ones_listed():
    assert list(om.MUTANTS) == ["gap_minus_one", "gap_plus_one", "last_feature_skipped", "feature_G_skipped",
                                "nesterov_mu_dropped", "rmsprop_v_not_decayed", "rmsprop_mom_row_held", "bias_skipped"]
    assert [d for d in om.DIMS if not om.MUTANTS["feature_G_skipped"][1](d)] == [1, 32]  # no element e = 1 there


@pytest.mark.parametrize("name", list(om.MUTANTS))
def test_every_mutant_is_caught_tenfold_among_the_gpu_cases(name):
    """At least one (kind, d, k) of the GPU grid shows the mutant at ten times a tolerance — and not at one dim only: some
    quantity shows it at EVERY dim the mutant exists at, and the defects that live in the rows (an edge feature or the
    bias left out, a lost factor) show there in the weights and in the logits both, so each layout's edges are held."""
    worst = {c: mutant_excess(name, *c) for c in cases_of(name)}
    best = max(worst.items(), key=lambda kv: max(kv[1].values()))
    print(f"{name}: largest excess {max(best[1].values()):.3g} at {best[0]}: "
          + ", ".join(f"{q} {x:.3g}" for q, x in best[1].items()))
    assert max(best[1].values()) >= 10.0, (name, best)
    in_rows = name not in ("gap_minus_one", "gap_plus_one", "rmsprop_v_not_decayed")  # those live in the state first
    for d in sorted({c[1] for c in worst}):
        at_d = [x for c, x in worst.items() if c[1] == d]
        assert max(max(x.values()) for x in at_d) >= 10.0, (name, d)
        if in_rows:
            assert max(x["weights"] for x in at_d) >= 10.0, (name, d)
            assert max(x["logits"] for x in at_d) >= 10.0, (name, d)


def test_a_skipped_edge_feature_shows_in_one_element_only():
    """What the table tolerance would miss if the step that follows hid it: the defect is one column wide."""
    for name, col in (("last_feature_skipped", lambda d: d - 1), ("feature_G_skipped", lambda d: om.layout(d)[0])):
        for d in (33, 300, 1000):
            sP, _ = tables("momentum", d)
            good, bad = om.replay_tables("momentum", sP, 7), om.MUTANTS[name][2]("momentum", sP, 7)
            diff = np.abs(good["w"] - bad["w"]).max(axis=0)
            assert diff[col(d)] > 10 * TOL and np.count_nonzero(diff) == 1
