"""Both lazy Adam replays (STRICT: opt_replay_row; batched stream: vo_replay) against the dense oracle, at the gates of
their closed forms and past the step at which the bias corrections saturate.

a. SEEDED STATE, EXACT GAPS.  The optimizer state of ~96 x 96 tables is written from tests/adam_replay_model.py's
   seeded rows (m = 0; typical; sqrt(v) at 0.1 ... 2x of each path's closed-form gate; rows with one element under
   the gate; lanes that also hold padding), the step counter is set to s0, and k steps touch three busy rows only.
   Every other row then owes exactly k zero-gradient steps s0+1 ... s0+k: the flush replays them WITH the state
   (k_flush_lazy / k_vflush), one more batch that touches every row replays them in the view and in the apply.  The
   reference is always `oracle.step` in its dense form from the same seeded state, for the closed form and for the
   step loop (set_tuning("adam_closed", 0)) alike — never the other route.  Before anything is launched the model says
   which seeded rows take which route, and the test asserts that the parameter set holds rows on both sides.
   tests/test_adam_replay_cpu.py shows without a GPU that these rows tell a right replay from a subtly wrong one.
b. A TRAINED TRAJECTORY past saturation on the batched stream (the counterpart of
   test_gpu_parity.test_adam_lazy_replay_long_gaps_after_warmup), with gap shares asserted from the schedule.
c. The 31-bit step limit of the batched stream, and set_step while its bookkeeping is live.

Tolerances: test_gpu_parity.close at 2e-5 (|err| <= 2e-5 max(1, |w|)) where only the replay acts; test_gpu_vstream.agree
(the same 2e-5, with close_mostly's few ill-conditioned elements) where a gradient step follows it.
"""
import functools

import numpy as np
import pytest

import adam_replay_model as am
import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402
from test_gpu_vstream import REG, agree, distinct_neg, oracle_opt  # noqa: E402

LR, EPS, TOL = 0.01, 1e-8, 2e-5
BETAS = [(0.9, 0.999), (0.1, 0.999)]
ROWS, B1 = 96, 16  # rows per table; batch size of the busy steps (>= 16: the direct form exists)
BUSY = (93, 94, 95)  # user, positive, negative of the busy steps: typical rows
STATE = ("mP", "vP", "mQ", "vQ", "mb", "vb")


def _cases():
    out = []
    for betas in BETAS:
        t_sat = am.host_consts(*betas)[1]
        pts = [(2, t_sat), (3, 40_000), (15, t_sat - 8), (16, t_sat), (17, 40_000), (175, t_sat - 200), (176, 40_000),
               (177, t_sat), (400, t_sat - 200), (400, 40_000), (16, 2000)]
        for n, (k, s0) in enumerate(pts):
            for p, path in enumerate(("strict", "batched")):
                d = (50, 128)[(n + p) % 2]  # item bias rides on d = 50
                out.append(pytest.param(path, betas, k, s0, d, id=f"{path}-b1_{betas[0]}-k{k}-s{s0}-d{d}"))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def seeded(d, betas):
    """The seeded tables of one (d, betas), read-only: dict P, Q, b (d = 50), the state, clsP, clsQ."""
    wP, mP, vP, cP = am.seeded_rows(ROWS, d, *betas, EPS, seed=d)
    wQ, mQ, vQ, cQ = am.seeded_rows(ROWS, d, *betas, EPS, seed=d + 1000)
    s = dict(P=wP, Q=wQ, mP=mP, vP=vP, mQ=mQ, vQ=vQ, clsP=cP, clsQ=cQ, b=None)
    if d == 50:
        wb, mb, vb, cb = am.seeded_rows(ROWS, 1, *betas, EPS, seed=d + 2000)
        s.update(b=wb[:, 0].copy(), mb=mb[:, 0].copy(), vb=vb[:, 0].copy(), clsb=cb)
    for a in s.values():
        if a is not None:
            a.setflags(write=False)
    assert all(c[r] == am.TYPICAL for c in (cP, cQ) for r in BUSY)
    return s


def busy_steps(k):
    n = k * B1
    return (np.full(n, BUSY[0], np.int32), np.full(n, BUSY[1], np.int32), np.full(n, BUSY[2], np.int32))


def touch_batch():
    """Every row but the pad row once as a user, once as a positive and once as a negative."""
    rng = np.random.default_rng(7)
    users = (rng.permutation(ROWS - 1) + 1).astype(np.int32)
    pos = (rng.permutation(ROWS - 1) + 1).astype(np.int32)
    neg = np.roll(pos, 1)
    return users, pos, neg


@functools.lru_cache(maxsize=None)
def reference(d, betas, s0, k):
    """The dense oracle from the seeded state: (after the k busy steps, after the touching batch), read-only dicts."""
    s = seeded(d, betas)
    cur = {n: (None if s.get(n) is None else s[n].copy()) for n in ("P", "Q", "b") + STATE}
    st = {n: cur[n] for n in STATE if cur[n] is not None}
    opt = oracle_opt(cfg_of(betas))
    u, p, j = busy_steps(k)
    for t in range(k):
        sl = slice(t * B1, (t + 1) * B1)
        oracle.step(cur["P"], cur["Q"], cur["b"], u[sl], p[sl], j[sl], opt, s0 + t + 1, st, REG)
    flushed = {n: (None if a is None else a.copy()) for n, a in cur.items()}
    oracle.step(cur["P"], cur["Q"], cur["b"], *touch_batch(), opt, s0 + k + 1, st, REG)
    for r in (flushed, cur):
        for a in r.values():
            if a is not None:
                a.setflags(write=False)
    return flushed, cur


def cfg_of(betas, lr=LR):
    return dict(kind=2, lr=lr, betas=betas, eps=EPS)


def seeded_engine(d, betas, s0, closed, direct=None):
    s = seeded(d, betas)
    e = make_engine(s["P"].copy(), s["Q"].copy(), None if s["b"] is None else s["b"].copy(), REG)
    e.set_optimizer(**cfg_of(betas))
    if not closed:
        e.set_tuning("adam_closed", 0)
    if direct is not None:
        e.set_tuning("vs_direct", direct)
    st = e.alloc_opt_state()
    for n in STATE:
        if st[n] is not None:
            st[n].copy_(dev(s[n].copy()))
    e.flush_lazy()
    e.set_step(s0)
    return e, st


def train(e, path, users, pos, neg, B):
    if path == "strict":
        e.train_strict(dev(users), dev(pos), B, sampler=0, neg=dev(neg))
    else:
        e.train_stream_batched(dev(users), dev(pos), B, sampler=0, neg=dev(neg), max_inflight=1)


def got_of(e, st):
    g = dict(P=e.P.cpu().numpy(), Q=e.Q.cpu().numpy(), b=None if e.item_bias is None else e.item_bias.cpu().numpy())
    g.update({n: (None if st[n] is None else st[n].cpu().numpy()) for n in STATE})
    return g


def assert_routes(path, betas, k, s0, d):
    """From the model alone: the parameter set holds rows on each side of the route decision it stands for."""
    s = seeded(d, betas)
    kmax, t_sat = am.host_consts(*betas)
    expect_closed = s0 >= t_sat and k >= am.path_kw(path, *betas)["closed_min"]
    counts = {}
    for tab in ("P", "Q"):
        c = am.route_counts(path, s["m" + tab], s["v" + tab], s["cls" + tab], d, s0, k, *betas, EPS)
        counts[tab] = c
        assert c["still"] >= 8 and c["loop"] >= 4 and c["below_gate"] >= 4, (tab, c)  # both routes see m = 0; the loop has work
        if expect_closed:  # rows above the gate, rows below it, rows with one lane below it
            assert c["closed"] >= 60, (tab, c)
        else:  # a short gap, or bias corrections still warm (s0 < t_sat; s0 + k may straddle t_sat): all by the loop
            assert c["closed"] == 0 and c["loop"] == ROWS - c["still"], (tab, c)
    regime = ("closed" if expect_closed else "loop-past-saturation" if s0 >= t_sat else
              "loop-straddling-t_sat" if s0 + k > t_sat else "loop-warm")
    print(f"routes {path} betas={betas} k={k} s0={s0} d={d}: {regime}",
          {t: {n: c[n] for n in ("closed", "loop", "below_gate", "still")} for t, c in counts.items()})
    return regime


def seeded_mask(cls):
    m = np.ones(ROWS, bool)
    m[list(BUSY)] = False
    return m


def rel_state_ok(got, want):
    """The decayed moments to 1e-4 RELATIVE: 2^(k log2 beta) in fp32 carries |k log2 beta| 2^-24 <= 3e-6 for k = 400,
    beta1 = 0.9, the oracle's own fp32 recurrence at most 400 roundings = 2.4e-5; values under fp32's normal range
    (beta1 = 0.1 after 40 steps) are exempt."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-30))


@pytest.mark.parametrize("path,betas,k,s0,d", CASES)
def test_flush_replays_exactly_k_steps_with_state(path, betas, k, s0, d):
    """k_flush_lazy / k_vflush with STATE replay of exactly k steps on every seeded row."""
    assert_routes(path, betas, k, s0, d)
    want, _ = reference(d, betas, s0, k)
    s = seeded(d, betas)
    for closed in (True, False):
        e, st = seeded_engine(d, betas, s0, closed)
        train(e, path, *busy_steps(k), B1)
        e.flush_lazy()
        assert e.step_count == s0 + k
        got = got_of(e, st)
        quiet = seeded_mask(None)
        for n in ("P", "Q", "b") + STATE:
            if want[n] is None:
                continue
            print(f"flush {path} closed={closed} {n}: maxerr {maxerr(got[n][quiet], want[n][quiet]):.3g}")
            assert close(got[n][quiet], want[n][quiet], TOL), (closed, n, maxerr(got[n][quiet], want[n][quiet]))
            if n in STATE:
                assert rel_state_ok(got[n][quiet], want[n][quiet]), (closed, n)
            if n in ("P", "Q", "b"):  # the three busy rows took k real steps: not the subject, held to close_mostly's cap
                assert maxerr(got[n][~quiet], want[n][~quiet]) <= 10 * LR, (closed, n, "busy rows")
        for tab in ("P", "Q"):  # m = 0: not moved at all
            still = (s["cls" + tab] == am.ZERO_M)
            assert np.array_equal(got[tab][still], s[tab][still]), (closed, tab)
        assert np.abs(want["P"] - s["P"]).max() > (0.05 if betas[0] == 0.9 and k >= 15 else 1e-3)


@pytest.mark.parametrize("path,betas,k,s0,d", CASES)
def test_touch_views_and_applies_across_a_gap_of_k(path, betas, k, s0, d):
    """One batch touching every seeded row after the k busy steps: the view and the close / direct apply see a gap of
    exactly k.  The batched stream runs deferred (vs_direct 0) and direct (1: the touching batch has 95 >= 16 triples and
    every user alone in it)."""
    assert_routes(path, betas, k, s0, d)
    _, want = reference(d, betas, s0, k)
    s = seeded(d, betas)
    cfg = cfg_of(betas)
    for closed in (True, False):
        for direct in ((0, 1) if path == "batched" else (None,)):
            e, st = seeded_engine(d, betas, s0, closed, direct)
            train(e, path, *busy_steps(k), B1)
            train(e, path, *touch_batch(), ROWS - 1)
            e.flush_lazy()
            assert e.step_count == s0 + k + 1
            got = got_of(e, st)
            for n in ("P", "Q", "b"):
                if want[n] is None:
                    continue
                print(f"touch {path} closed={closed} direct={direct} {n}: maxerr {maxerr(got[n], want[n]):.3g}")
                assert agree(got[n], want[n], cfg), (closed, direct, n, maxerr(got[n], want[n]))
                # close_mostly's exemptions are for gradients that sum to ~0: none on the m = 0 and typical rows
                cls = s["cls" + n] if n != "b" else s["clsb"]
                plain = seeded_mask(None) & ((cls == am.ZERO_M) | (cls == am.TYPICAL))
                err = np.abs(got[n][plain] - want[n][plain]) / np.maximum(1.0, np.abs(want[n][plain]))
                assert int((err > TOL).sum()) == 0, (closed, direct, n, int((err > TOL).sum()), err.max())
            assert not got["P"][0].any()


# ---- b. a trained trajectory past saturation on the batched stream ---------------------------------------------------
TU, TI, TB, T0, TSTEPS = 1200, 800, 16, 40_000, 400
TREG = (0.002, 0.001, 0.003)


@functools.lru_cache(maxsize=None)
def trajectory_schedule():
    rng = np.random.default_rng(11)
    warm = [(rng.integers(1, TU, 2000).astype(np.int32), rng.integers(1, TI, 2000).astype(np.int32)) for _ in range(3)]
    warm = [(u, p, distinct_neg(p, rng.integers(1, TI, 2000).astype(np.int32), TI)) for u, p in warm]
    n = TSTEPS * TB
    u, p = rng.integers(1, TU, n).astype(np.int32), rng.integers(1, TI, n).astype(np.int32)
    return warm, (u, p, distinct_neg(p, rng.integers(1, TI, n).astype(np.int32), TI))


def gap_shares(users, pos, neg, B, U, I):
    """Shares of row touches (a row once per batch) whose row sat untouched for >= 16 and for > 176 steps."""
    lastP, lastQ = np.zeros(U, np.int64), np.zeros(I, np.int64)
    gaps = []
    for t in range(len(users) // B):
        sl = slice(t * B, (t + 1) * B)
        for last, rows in ((lastP, np.unique(users[sl])), (lastQ, np.unique(np.concatenate([pos[sl], neg[sl]])))):
            gaps.append(t - last[rows])  # zero-gradient steps owed at this touch
            last[rows] = t + 1
    gaps = np.concatenate(gaps)
    return float((gaps >= 16).mean()), float((gaps > 176).mean())


@functools.lru_cache(maxsize=None)
def trajectory_reference(d, bias, betas):
    warm, (u, p, j) = trajectory_schedule()
    rng = np.random.default_rng(d)
    P = ((rng.random((TU, d)) - 0.5) / d * 16).astype(np.float32)
    Q = ((rng.random((TI, d)) - 0.5) / d * 16).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b = np.linspace(-0.1, 0.1, TI).astype(np.float32) if bias else None
    Po, Qo, bo = P.copy(), Q.copy(), None if b is None else b.copy()
    st = {k: np.zeros_like(Po if k.endswith("P") else Qo) for k in ("mP", "vP", "mQ", "vQ")}
    if bias:
        st["mb"], st["vb"] = np.zeros_like(b), np.zeros_like(b)
    opt = oracle_opt(cfg_of(betas, 0.003))
    for t, (wu, wp, wj) in enumerate(warm):
        oracle.step(Po, Qo, bo, wu, wp, wj, opt, t + 1, st, TREG)
    for t in range(TSTEPS):
        sl = slice(t * TB, (t + 1) * TB)
        oracle.step(Po, Qo, bo, u[sl], p[sl], j[sl], opt, T0 + 1 + t, st, TREG)
    for a in (P, Q, b, Po, Qo, bo):
        if a is not None:
            a.setflags(write=False)
    return P, Q, b, Po, Qo, bo


def test_trajectory_schedule_has_the_long_gaps():
    _, (u, p, j) = trajectory_schedule()
    ge16, gt176 = gap_shares(u, p, j, TB, TU, TI)
    print(f"gap shares: >= 16: {ge16:.3f}, > 176: {gt176:.4f}")
    assert ge16 >= 0.30 and gt176 >= 0.005, (ge16, gt176)


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("route", ["closed", "loop"])
@pytest.mark.parametrize("d,bias,betas", [(50, True, BETAS[0]), (128, False, BETAS[0]), (256, False, BETAS[0]),
                                          (128, False, BETAS[1])])
def test_batched_stream_trajectory_past_saturation(d, bias, betas, route, direct):
    """400 batches of 16 on 1,200 x 800 tables, 40,000 steps into training, max_inflight = 1: most touches replay
    16+ steps, some more than kmax = 176, in the view and in the apply, by the series or by the saturated step loop."""
    warm, (u, p, j) = trajectory_schedule()
    ge16, gt176 = gap_shares(u, p, j, TB, TU, TI)
    assert ge16 >= 0.30 and gt176 >= 0.005, (ge16, gt176)
    P, Q, b, Po, Qo, bo = trajectory_reference(d, bias, betas)
    cfg = cfg_of(betas, 0.003)
    e = make_engine(P.copy(), Q.copy(), None if b is None else b.copy(), TREG)
    e.set_optimizer(**cfg)
    e.set_tuning("vs_direct", direct)
    if route == "loop":
        e.set_tuning("adam_closed", 0)
    e.alloc_opt_state()
    for wu, wp, wj in warm:
        e.train_stream_batched(dev(wu), dev(wp), 2000, sampler=0, neg=dev(wj), max_inflight=1)
    e.flush_lazy()
    e.set_step(T0)
    cut = 170 * TB  # two launches: pending steps and headers carry across
    e.train_stream_batched(dev(u[:cut]), dev(p[:cut]), TB, sampler=0, neg=dev(j[:cut]), max_inflight=1)
    e.train_stream_batched(dev(u[cut:]), dev(p[cut:]), TB, sampler=0, neg=dev(j[cut:]), max_inflight=1)
    e.flush_lazy()
    assert e.step_count == T0 + TSTEPS
    Pg, Qg = e.P.cpu().numpy(), e.Q.cpu().numpy()
    print(f"trajectory d={d} betas={betas} {route} direct={direct}: maxerr P {maxerr(Pg, Po):.3g} Q {maxerr(Qg, Qo):.3g}")
    assert np.abs(Po - P).max() > 0.01 and np.abs(Qo - Q).max() > 0.01  # the tables really moved
    assert agree(Pg, Po, cfg, TOL), maxerr(Pg, Po)
    assert agree(Qg, Qo, cfg, TOL), maxerr(Qg, Qo)
    if bias:
        assert agree(e.item_bias.cpu().numpy(), bo, cfg, TOL)


# ---- c. small things -------------------------------------------------------------------------------------------------
def test_batched_stream_refuses_steps_past_31_bits_and_launches_nothing():
    from revisit_bpr import native

    s = seeded(128, BETAS[0])
    e, st = seeded_engine(128, BETAS[0], 2 ** 31 - 2, True)
    u, p, j = touch_batch()
    with pytest.raises(native.BprError) as err:
        e.train_stream_batched(dev(u), dev(p), 16, sampler=0, neg=dev(j), max_inflight=1)
    assert err.value.code == -3  # BPR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert e.step_count == 2 ** 31 - 2
    got = got_of(e, st)
    for n in ("P", "Q") + STATE[:4]:
        assert np.array_equal(got[n], s[n]), n


@pytest.mark.parametrize("pending", [False, True])
def test_set_step_while_the_batched_bookkeeping_is_live_flushes_every_row(pending):
    """set_step with headers live (rows stale, and — pending — steps parked in the accumulators): P and Q afterwards
    are what flush_lazy gives, and a later flush finds nothing left to do."""
    d, betas, s0, k = 128, BETAS[0], 40_000, 17
    out = []
    for how in ("set_step", "flush"):
        e, st = seeded_engine(d, betas, s0, True)
        train(e, "batched", *busy_steps(k), B1)
        if pending:
            train(e, "batched", *touch_batch(), ROWS - 1)
        if how == "set_step":
            e.set_step(s0 + 1000)
            assert e.step_count == s0 + 1000
            before = (e.P.clone(), e.Q.clone())
            e.flush_lazy()  # every row is current as of the new step: nothing moves
            assert torch.equal(before[0], e.P) and torch.equal(before[1], e.Q)
        else:
            e.flush_lazy()
        out.append(got_of(e, st))
    for n in ("P", "Q") + STATE[:4]:
        assert np.array_equal(out[0][n], out[1][n]), n
    want = reference(d, betas, s0, k)[1 if pending else 0]
    assert agree(out[0]["P"], want["P"], cfg_of(betas)) and agree(out[0]["Q"], want["Q"], cfg_of(betas))
