"""The STRICT kernels' lazy replay under every stateful optimizer against the dense oracle, at all six row layouts.

`bpr_bind_tables` picks (G lanes per row, E elements per lane) from the embedding dim; k_triples, k_apply and
k_flush_lazy exist once per layout, and under a stateful optimizer they replay the zero-gradient steps a dense
torch.optim applied to rows nobody touched: `opt_replay_row` for a row, `opt_replay` for an item bias, `catch_up_row`
for the view the forward pass reads.  tests/opt_replay_model.py's DIMS put every layout at its edges (smallest d, largest
d but for (32,4), a partial last element, one lane holding the whole row); here each of them runs

  * momentum, Nesterov, dampening, RMSprop and RMSprop with momentum from opt_replay_model.seeded_state, 1000 steps into
    training, over gaps of 1, 7 and 60 steps;
  * Adam from adam_replay_model.seeded_rows at d = 1, 64, 200, 300, 1000, on both sides of its closed-form gates,
    with the closed form on and off.

The pattern is test_gpu_adam_replay.py's: the seeded state is written into the engine, the step counter set, k steps
touch three busy rows only, and every other row then owes exactly k zero-gradient steps.  A flush replays them WITH the
state; one batch that touches every row replays them in the view (its LOGITS are compared: a single element replayed
wrongly in the view shows there, while it reaches the tables only through sigma(-x) times lr) and in the apply.  That
batch also holds the pad user, the pad item as a positive and the pad item as a negative.  The only reference is
`oracle.step` in its dense form from the same seeded state.  tests/test_opt_replay_cpu.py shows without a GPU that the
seeded tables tell a right replay from a wrong one with a tenfold margin.

Tolerances are the suite's: test_gpu_parity.close at 2e-5 (|err| <= 2e-5 max(1, |w|)) for weights and logits,
test_gpu_adam_replay.rel_state_ok (1e-4 relative, derived there for 400 steps) for the state, test_gpu_vstream.agree
where a gradient step follows the replay.
"""
import functools

import numpy as np
import pytest

import adam_replay_model as am
import opt_replay_model as om

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_adam_replay import (B1, BETAS, BUSY, EPS, ROWS, STATE, busy_steps, cfg_of, got_of,  # noqa: E402
                                  rel_state_ok)
from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402
from test_gpu_vstream import REG, agree  # noqa: E402
from test_opt_replay_cpu import (QUIET, S0, as_engine, dense_reference, oracle_opt, reference, tables,  # noqa: E402
                                 touch_batch_with_pads)

TOL = 2e-5
assert ROWS == om.ROWS


def engine_from(seeded, cfg, s0, closed=True):
    """A fresh engine holding the seeded tables and state (names as test_opt_replay_cpu.as_engine), s0 steps in."""
    e = make_engine(seeded["P"].copy(), seeded["Q"].copy(), seeded["b"].copy(), REG)
    e.set_optimizer(**cfg)
    if not closed:
        e.set_tuning("adam_closed", 0)
    st = e.alloc_opt_state()
    for n in STATE:
        assert (st[n] is None) == (seeded[n] is None), n
        if st[n] is not None:
            st[n].copy_(dev(seeded[n].copy()))
    e.flush_lazy()
    e.set_step(s0)
    return e, st


def run_busy(e, k):
    u, p, j = busy_steps(k)
    e.train_strict(dev(u), dev(p), B1, sampler=0, neg=dev(j))


def touch(e):
    """The touching batch as ONE bpr_step; returns its logits."""
    lp, ln, _, _ = e.step(*(dev(a) for a in touch_batch_with_pads()))
    return lp.cpu().numpy(), ln.cpu().numpy()


def check_flush(tag, got, want, seeded, still, lr):
    """After the flush: weights and state of the quiet rows against the dense oracle; m = 0 rows bit-equal."""
    for n in ("P", "Q", "b") + STATE:
        if want[n] is None:
            assert got[n] is None, n
            continue
        print(f"flush {tag} {n}: maxerr {maxerr(got[n][QUIET], want[n][QUIET]):.3g}")
        assert close(got[n][QUIET], want[n][QUIET], TOL), (n, maxerr(got[n][QUIET], want[n][QUIET]))
        if n in STATE:
            assert rel_state_ok(got[n][QUIET], want[n][QUIET]), n
        else:  # the three busy rows took k real steps: not the subject, held to close_mostly's cap
            assert maxerr(got[n][~QUIET], want[n][~QUIET]) <= 10 * lr, (n, "busy rows")
    for n in ("P", "Q", "b"):
        assert np.array_equal(got[n][still[n]], seeded[n][still[n]]), (n, "m = 0 rows moved")


def check_touch(tag, got, logits, want, cfg, plain):
    """After the touching batch and a flush: its logits (the view), then the tables (the apply)."""
    for n, x in zip(("lp", "ln"), logits):
        print(f"touch {tag} {n}: maxerr {maxerr(x, want[n]):.3g}")
        assert close(x, want[n], TOL), (n, maxerr(x, want[n]))
    for n in ("P", "Q", "b"):
        print(f"touch {tag} {n}: maxerr {maxerr(got[n], want[n]):.3g}")
        assert agree(got[n], want[n], cfg), (n, maxerr(got[n], want[n]))
        # close_mostly's exemptions are for gradients that sum to ~0 under a division by sqrt(v) ~ |g|: none here
        err = np.abs(got[n][plain[n]] - want[n][plain[n]]) / np.maximum(1.0, np.abs(want[n][plain[n]]))
        assert int((err > TOL).sum()) == 0, (n, int((err > TOL).sum()), err.max())
    assert not got["P"][0].any() and not got["Q"][0].any()
    assert close(got["b"][0], want["b"][0], TOL)


# ---- momentum, Nesterov, dampening, RMSprop, RMSprop with momentum ---------------------------------------------------
GRID = [pytest.param(kind, d, k, id=f"{kind}-d{d}-k{k}") for kind in om.KINDS for d in om.DIMS for k in om.GAPS]


@pytest.mark.parametrize("kind,d,k", GRID)
def test_flush_replays_k_steps_with_state(kind, d, k):
    """k_flush_lazy<G, E>: opt_replay_row with STATE and opt_replay of the bias, over a gap of exactly k."""
    sP, sQ = tables(kind, d)
    seeded, cfg = as_engine(sP, sQ), om.KINDS[kind]
    want, _ = reference(kind, d, k)
    e, st = engine_from(seeded, cfg, S0)
    run_busy(e, k)
    e.flush_lazy()
    assert e.step_count == S0 + k
    got = got_of(e, st)
    # rows that must stay bit-equal: m = 0; under plain RMSprop a zero gradient moves no weight at all, only v decays
    still = dict(P=sP["still"], Q=sQ["still"], b=sQ["still_b"]) if om.has_m(kind) else dict(P=QUIET, Q=QUIET, b=QUIET)
    check_flush(f"{kind} d={d} k={k} layout={om.layout(d)}", got, want, seeded, still, cfg["lr"])
    # not vacuous: the reference moved the quiet rows by more than 1e-3 somewhere (under plain RMSprop, their v)
    moved = "P" if om.has_m(kind) else "vP"
    assert np.abs(want[moved][QUIET].astype(np.float64) - seeded[moved][QUIET]).max() > 1e-3


@pytest.mark.parametrize("kind,d,k", GRID)
def test_touch_views_and_applies_across_a_gap(kind, d, k):
    """k_triples<G, E>: catch_up_row and the bias view over a gap of k, held by the logits; then k_apply<G, E>."""
    sP, sQ = tables(kind, d)
    seeded, cfg = as_engine(sP, sQ), om.KINDS[kind]
    _, want = reference(kind, d, k)
    e, st = engine_from(seeded, cfg, S0)
    run_busy(e, k)
    logits = touch(e)
    e.flush_lazy()
    assert e.step_count == S0 + k + 1
    # every seeded row is an m = 0 row or a typical row: all quiet rows are held without exceptions
    check_touch(f"{kind} d={d} k={k} layout={om.layout(d)}", got_of(e, st), logits, want, cfg, dict(P=QUIET, Q=QUIET, b=QUIET))


# ---- Adam at the layouts test_gpu_adam_replay.py (d = 50, 128) does not reach -----------------------------------------
def _adam_cases():
    out = []
    for betas in BETAS:
        t_sat = am.host_consts(*betas)[1]
        for k, s0 in ((3, 40_000), (16, t_sat), (177, t_sat), (400, t_sat - 200)):
            for d in (1, 64, 200, 300, 1000):
                for closed in (True, False):
                    out.append(pytest.param(betas, k, s0, d, closed, id=f"b1_{betas[0]}-k{k}-s{s0}-d{d}-closed{int(closed)}"))
    return out


@functools.lru_cache(maxsize=None)
def adam_seeded(d, betas):
    """adam_replay_model.seeded_rows for P, Q and the item bias (at every d), read-only, with the row classes."""
    wP, mP, vP, cP = am.seeded_rows(ROWS, d, *betas, EPS, seed=d)
    wQ, mQ, vQ, cQ = am.seeded_rows(ROWS, d, *betas, EPS, seed=d + 1000)
    wb, mb, vb, cb = am.seeded_rows(ROWS, 1, *betas, EPS, seed=d + 2000)
    s = dict(P=wP, Q=wQ, b=wb[:, 0].copy(), mP=mP, vP=vP, mQ=mQ, vQ=vQ, mb=mb[:, 0].copy(), vb=vb[:, 0].copy())
    cls = dict(P=cP, Q=cQ, b=cb)
    for a in list(s.values()) + list(cls.values()):
        a.setflags(write=False)
    assert all(c[r] == am.TYPICAL for c in cls.values() for r in BUSY)
    return s, cls


@functools.lru_cache(maxsize=None)
def adam_reference(d, betas, s0, k):
    return dense_reference(adam_seeded(d, betas)[0], oracle_opt(cfg_of(betas)), s0, k)


def assert_adam_routes(betas, k, s0, d):
    """test_gpu_adam_replay.assert_routes for these tables: from the model alone, rows on both sides of the decision."""
    s, cls = adam_seeded(d, betas)
    _, t_sat = am.host_consts(*betas)
    expect_closed = s0 >= t_sat and k >= am.path_kw("strict", *betas)["closed_min"]
    for tab in ("P", "Q"):
        c = am.route_counts("strict", s["m" + tab], s["v" + tab], cls[tab], d, s0, k, *betas, EPS)
        assert c["still"] >= 8 and c["loop"] >= 4 and c["below_gate"] >= 4, (tab, c)
        if expect_closed:
            # d = 1: a row IS one element, so a row below the gate has nothing above it.  Of 96 rows 8 are still and
            # 7 sit under the STRICT gate (three gate rows, four mixed rows); the other 81 take the series, so the
            # count of 60 holds there too and nothing needs relaxing.
            assert c["closed"] >= 60, (tab, c)
        else:
            assert c["closed"] == 0 and c["loop"] == ROWS - c["still"], (tab, c)
        print(f"routes betas={betas} k={k} s0={s0} d={d} {tab}:", {n: c[n] for n in ("closed", "loop", "below_gate", "still")})


@pytest.mark.parametrize("betas,k,s0,d,closed", _adam_cases())
def test_adam_at_the_other_layouts(betas, k, s0, d, closed):
    """The flush and the touch of test_gpu_adam_replay.py (path "strict") at the layouts (32,1) with one live lane,
    (32,2) full, (64,4), (64,8) and (64,16) with partial last elements, item bias on, plus the logits of the touch."""
    assert_adam_routes(betas, k, s0, d)
    seeded, cls = adam_seeded(d, betas)
    flushed, touched = adam_reference(d, betas, s0, k)
    cfg = cfg_of(betas)
    tag = f"adam betas={betas} k={k} s0={s0} d={d} layout={om.layout(d)} closed={closed}"

    e, st = engine_from(seeded, cfg, s0, closed)
    run_busy(e, k)
    e.flush_lazy()
    assert e.step_count == s0 + k
    check_flush(tag, got_of(e, st), flushed, seeded, {n: c == am.ZERO_M for n, c in cls.items()}, cfg["lr"])
    assert np.abs(flushed["P"] - seeded["P"]).max() > (0.05 if betas[0] == 0.9 and k >= 15 else 1e-3)

    e, st = engine_from(seeded, cfg, s0, closed)
    run_busy(e, k)
    logits = touch(e)
    e.flush_lazy()
    assert e.step_count == s0 + k + 1
    plain = {n: QUIET & ((c == am.ZERO_M) | (c == am.TYPICAL)) for n, c in cls.items()}
    check_touch(tag, got_of(e, st), logits, touched, cfg, plain)
