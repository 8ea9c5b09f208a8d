"""Fold-in with scored negatives on the GPU: `bpr_fold_in_rows_scored` (revisit-bpr_amd/csrc/bpr_foldin_scored.hip) and
what is built on it (revisit_bpr.foldin.fold_in(sampler="dynamic" | "warp"), Engine.fold_in, Model.fold_in).

The draws are held to the library's own stand-alone samplers, bit for bit, at the row state the kernel reports through
its test hook (1, 5); the dynamic update to the existing given-negative kernel, bit for bit (2); the WARP update to a
float64 step within a bound derived from its roundings (3); the whole run to the numpy restatement of
tests/foldin_scored_model.py on cases that tests/test_foldin_scored_cpu.py has shown to be decided (4).  Epochs chain
(6), the result is a pure function of its definition (7), WARP takes the first violator and dynamic the best (8), nothing
else is written (9), and the Engine / Model entry points are the free function (10).

The engine's group shape for a width d is `group_shape(d)`, the one `foldin_ge(d)` gives (bpr_group_shape.h: one
function), so the stand-alone samplers reduce in the kernel's order at every d here."""
import ctypes

import numpy as np
import pytest
import torch

import dynamic_model as dm
import foldin_scored_model as fm
import warp_model as wm

pytestmark = pytest.mark.gpu

LR, MARGIN, SEED, OFFSET = fm.LR, fm.MARGIN, fm.SEED, fm.OFFSET
DIMS = [8, 33, 128, 300, 1024]  # E = 1 and E = 2 at G = 32, E = 4 full; a partial E = 8 and a full E = 16 at G = 64
ITEMS = [50, 300]
KS = [1, 4, 10, 32]
KINDS = ["dynamic", "warp"]
DYNAMIC, WARP = 3, 4


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Case:
    """Tables, histories and initial rows for one (I, d); built once, never changed."""

    def __init__(self, I, d, seed=0):
        pr = fm.problem(I, d, seed)
        self.pr, self.I, self.d, self.lens, self.rows = pr, I, d, pr["lens"], pr["rows"]
        self.indptr, self.items, self.n, self.nnz = pr["indptr"], pr["items"], pr["n"], pr["nnz"]
        self.Q, self.b, self.P0 = gpu(pr["Q"]), gpu(pr["b"]), gpu(pr["P0"])
        self.g_indptr, self.g_items = gpu(self.indptr), gpu(self.items)
        self.users_of = np.repeat(np.arange(self.n), self.lens).astype(np.int32)  # row of CSR position k

    def fold(self, kind, K, epochs=1, bias=True, reg=0.05, lr=LR, init=None, offset=OFFSET, **kw):
        from revisit_bpr.foldin import fold_in

        out = fold_in(self.Q, self.b if bias else None, kw.pop("indptr", self.g_indptr), self.g_items, epochs=epochs,
                      lr=lr, reg_user=reg, init=self.P0 if init is None else init, seed=SEED, offset=offset,
                      sampler=kind, candidates=K, max_sampled=K, margin=MARGIN, return_neg=True, return_draws=True, **kw)
        torch.cuda.synchronize()
        return out

    def sampler_engine(self, P, indptr, indices, bias=True):
        from revisit_bpr import engine as eng

        e = eng.Engine(P.contiguous(), self.Q.clone(), self.b.clone() if bias else None, pad_user=None)
        e.bind_seen_csr(gpu(indptr), gpu(indices))
        return e

    def engine_draws(self, e, kind, K, users, pos, offset=OFFSET):
        if kind == "dynamic":
            neg = e.sample_dynamic(users, K, SEED, offset)
            out = (neg, torch.zeros_like(neg))
        else:
            out = e.sample_warp(users, pos, K, SEED, offset, margin=MARGIN)
        torch.cuda.synchronize()
        return out


_cases = {}


def case(I, d):
    if (I, d) not in _cases:
        _cases[(I, d)] = Case(I, d)
    return _cases[(I, d)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def mismatch(name, got, ref):
    bad = torch.nonzero(got != ref).reshape(-1)
    assert bad.numel() == 0, (name, bad[:5].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())


# ---- 1. every draw is the stand-alone sampler's at the state it saw ------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_draw_is_the_stand_alone_samplers_at_the_state_it_saw(kind, I, d, bias):
    c = case(I, d)
    seen_indptr = np.concatenate([[0], np.cumsum([c.lens[r] for r in c.users_of])]).astype(np.int64)
    seen = np.concatenate([c.rows[r] for r in c.users_of]).astype(np.int32)
    users = torch.arange(c.nnz, dtype=torch.int32, device="cuda")
    early = late = skips = 0
    for K in KS:
        P, neg, tries, states = c.fold(kind, K, bias=bias, _states=True)
        assert tuple(states.shape) == (c.nnz, c.d)
        # pseudo-user t: row = the state the draw of triple t saw, seen = the WHOLE history of its row
        e = c.sampler_engine(states, seen_indptr, seen, bias)
        want = c.engine_draws(e, kind, K, users, c.g_items)
        mismatch("negative", neg, want[0])
        mismatch("tries", tries, want[1])
        e.close()
        neg_h, tries_h = neg.cpu().numpy(), tries.cpu().numpy()
        # the first state of a row is its init, and the two rows whose answer is known without any sampler
        for r in range(c.n):
            if c.lens[r]:
                assert torch.equal(states[int(c.indptr[r])], c.P0[r])
        lo, hi = int(c.indptr[-3]), int(c.indptr[-2])
        only = np.setdiff1d(np.arange(1, I), c.rows[-2])
        assert len(only) == 1
        if kind == "dynamic":
            assert (neg_h[lo:hi] == only[0]).all() and (neg_h[hi:] == 0).all() and (tries_h == 0).all()
        else:
            assert set(neg_h[lo:hi].tolist()) <= {int(only[0]), -1} and (neg_h[hi:] <= 0).all()
            assert ((neg_h == -1) == (tries_h == 0)).all() and tries_h.max() <= K
            early, late, skips = early + (tries_h == 1).sum(), late + (tries_h > 1).sum(), skips + (neg_h == -1).sum()
        assert torch.equal(P[-1], c.P0[-1]) and torch.equal(P[0], c.P0[0])  # all seen: every triple skipped; no triple
        for r in range(1, c.n - 1):  # every other pick is an unseen item of its row
            for j in neg_h[c.indptr[r]:c.indptr[r + 1]]:
                assert j == -1 or (1 <= j < I and j not in c.rows[r])
    if kind == "warp":
        assert early > 0 and late > 0 and skips > 0, (early, late, skips)


# ---- 2. the dynamic update is the existing kernel's --------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_dynamic_rows_are_the_given_negative_kernels_on_the_picks(I, d, bias, reg):
    from revisit_bpr.foldin import fold_in

    c = case(I, d)
    for K in (4, 32):
        P, neg, tries = c.fold("dynamic", K, epochs=3, bias=bias, reg=reg)
        assert neg.shape == (3 * c.nnz,) and int(tries.abs().max()) == 0
        want = fold_in(c.Q, c.b if bias else None, c.g_indptr, c.g_items, epochs=3, lr=LR, reg_user=reg, init=c.P0, neg=neg)
        assert torch.equal(P, want)
        assert torch.equal(P[0], c.P0[0]) and torch.equal(P[-1], c.P0[-1])
        assert all(not torch.equal(P[r], c.P0[r]) for r in range(1, c.n - 1))


# ---- 3. the WARP update, step by step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_warp_update_step_by_step(I, d, reg):
    """states[t'] (t' the row's next triple) against the float64 step from states[t] with the kernel's own pick and
    warp_model.weight.  The kernel computes p + (-lr) * ((-L) * (q_i - q_j) + au * p) without contraction: six fp32
    roundings (difference, two products, sum, product, sum), each at most 2^-24 relative on a partial result no larger
    than |p| + lr (L |q_i - q_j| + au |p|); logf is within 2 ulp of log, which the constant 8 still covers.  A skipped
    triple's next state is bit-equal; L = 0 moves the row by the L2 term only."""
    c = case(I, d)
    epochs, K = 2, 4
    P, neg, tries, states = c.fold("warp", K, epochs=epochs, reg=reg, _states=True)
    neg_h, tries_h, S = neg.cpu().numpy(), tries.cpu().numpy(), states.cpu().numpy()
    Q, Pf = c.pr["Q"].astype(np.float64), P.cpu().numpy()
    stepped = skipped = l2_only = 0
    for r in range(c.n):
        m, lo = c.lens[r], int(c.indptr[r])
        ts = [e * c.nnz + lo + k for e in range(epochs) for k in range(m)]
        for a, t in enumerate(ts):
            nxt = S[ts[a + 1]] if a + 1 < len(ts) else Pf[r]
            i, j = int(c.items[t % c.nnz]), int(neg_h[t])
            if j < 1:
                assert np.array_equal(nxt, S[t]), (r, t)
                skipped += 1
                continue
            L = wm.weight((I - 1) - m, int(tries_h[t]))
            p = S[t].astype(np.float64)
            want = p - LR * (-L * (Q[i] - Q[j]) + reg * p)
            bound = 8 * 2.0 ** -24 * (np.abs(p) + LR * (L * np.abs(Q[i] - Q[j]) + reg * np.abs(p)))
            assert (np.abs(nxt - want) <= bound).all(), (r, t, float(np.abs(nxt - want).max()), float(bound.max()))
            stepped += 1
            if L == 0.0:
                l2_only += 1
                assert m == I - 2 or tries_h[t] > ((I - 1) - m) / 2
                if reg == 0.0:
                    assert np.array_equal(nxt, S[t])
    assert stepped > 0 and skipped > 0 and l2_only > 0


# ---- 4. the whole run against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("I, d, N", sorted(fm.RUN_SEED))
@pytest.mark.parametrize("kind", KINDS)
def test_free_running_against_the_restatement(kind, I, d, N):
    from revisit_bpr.foldin import fold_in

    pr, (P, neg, tries, und) = fm.run_model(kind, I, d, N)
    assert not und.any()
    got = fold_in(gpu(pr["Q"]), gpu(pr["b"]), gpu(pr["indptr"]), gpu(pr["items"]), epochs=fm.RUN_EPOCHS, lr=fm.LR,
                  reg_user=fm.REG, init=gpu(pr["P0"]), seed=fm.SEED, offset=fm.OFFSET, sampler=kind, candidates=N,
                  max_sampled=N, margin=fm.MARGIN, return_neg=True, return_draws=True)
    torch.cuda.synchronize()
    assert np.array_equal(got[1].cpu().numpy(), neg) and np.array_equal(got[2].cpu().numpy(), tries)
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - P).max()
    print(f"{kind} I={I} d={d} N={N}: max |row - model| = {err:.3e}")
    assert err <= 1e-5


# ---- 5. lr = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_with_lr_zero_every_draw_is_the_samplers_on_the_initial_row(kind, I, d):
    c = case(I, d)
    epochs, K = 4, 10
    P, neg, tries = c.fold(kind, K, epochs=epochs, lr=0.0, reg=0.0)
    assert torch.equal(P, c.P0)
    e = c.sampler_engine(c.P0.clone(), c.indptr, c.items)
    want = c.engine_draws(e, kind, K, gpu(np.tile(c.users_of, epochs)), gpu(np.tile(c.items, epochs)))
    e.close()
    mismatch("negative", neg, want[0])
    mismatch("tries", tries, want[1])
    per_epoch = neg.reshape(epochs, c.nnz)
    assert not torch.equal(per_epoch[0], per_epoch[1])  # (different counters draw differently)


# ---- 6. epochs chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_three_epochs_are_three_calls_of_one(kind, I, d):
    c = case(I, d)
    P, neg, tries = c.fold(kind, 4, epochs=3)
    Pe, parts = c.P0, []
    for e in range(3):
        Pe, *draws = c.fold(kind, 4, epochs=1, init=Pe, offset=OFFSET + e * c.nnz)
        parts.append(draws)
    assert torch.equal(P, Pe)
    for k, whole in enumerate((neg, tries)):
        assert torch.equal(whole, torch.cat([part[k] for part in parts]))


# ---- 7. a pure function ------------------------------------------------------------------------------------------------
def raw(c, kind, K, row_order=None, epochs=3, seen_mode=0, pad=0):
    """The entry point itself (through the test hook): any row_order, the seen structure forced, `pad` sentinel words
    around P_new, neg_out and tries_out."""
    from revisit_bpr import native

    fn = native.load().bpr_test_fold_in_rows_scored
    fn.restype = ctypes.c_int
    fn.argtypes = native.SIGNATURES["bpr_fold_in_rows_scored"][1] + [ctypes.c_int32, ctypes.c_void_p]
    Pbuf = torch.full((c.n * c.d + 2 * pad,), -7.5, dtype=torch.float32, device="cuda")
    Pbuf[pad:pad + c.n * c.d] = c.P0.reshape(-1)
    outs = [torch.full((epochs * c.nnz + 2 * pad,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    native.check(fn(c.Q.data_ptr(), c.b.data_ptr(), c.I, c.d, c.g_indptr.data_ptr(), c.g_items.data_ptr(), c.n,
                    None if row_order is None else row_order.data_ptr(), epochs, LR, 0.05, WARP if kind == "warp" else DYNAMIC,
                    K, MARGIN, outs[0].data_ptr() + 4 * pad, outs[1].data_ptr() + 4 * pad, SEED, OFFSET,
                    Pbuf.data_ptr() + 4 * pad, torch.cuda.current_stream().cuda_stream, seen_mode, None))
    torch.cuda.synchronize()
    return Pbuf, outs[0], outs[1]


def inner(bufs, c, epochs, pad):
    return (bufs[0][pad:pad + c.n * c.d].reshape(c.n, c.d), bufs[1][pad:pad + epochs * c.nnz],
            bufs[2][pad:pad + epochs * c.nnz])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_result_does_not_depend_on_order_balance_seen_structure_or_call(kind, I, d):
    c = case(I, d)
    K = 10
    base = c.fold(kind, K, epochs=3)
    rng = np.random.default_rng(3)
    desc = gpu(np.argsort(-np.asarray(c.lens), kind="stable").astype(np.int32))
    for row_order in (None, desc, gpu(rng.permutation(c.n).astype(np.int32))):
        for seen_mode in (0, 1, 2):
            got = inner(raw(c, kind, K, row_order, seen_mode=seen_mode), c, 3, 0)
            assert same(got, base), (row_order, seen_mode)
            assert int(got[1].min()) >= -1 and int(got[2].min()) >= 0  # every entry written
    for seen_mode in (1, 2):
        assert same(c.fold(kind, K, epochs=3, _seen_mode=seen_mode), base)
    for balance in (True, False):
        assert same(c.fold(kind, K, epochs=3, balance=balance), base)
    # one call against two half calls: CSR slices, the counter advanced to keep t (epochs = 1)
    whole = c.fold(kind, K, epochs=1)
    for a, z in ((0, 5), (5, c.n)):
        lo, hi = int(c.indptr[a]), int(c.indptr[z])
        half = c.fold(kind, K, epochs=1, indptr=c.g_indptr[a:z + 1], init=c.P0[a:z], offset=OFFSET + lo)
        assert torch.equal(half[0], whole[0][a:z])
        assert all(torch.equal(half[k], whole[k][lo:hi]) for k in (1, 2))


@pytest.mark.parametrize("kind", KINDS)
def test_a_large_catalogue_takes_the_csr_by_itself(kind):
    """I = 70,000 at d = 32: eight bitmaps do not fit 64 KiB, the plan chooses the row's CSR slice, and the draws are
    still the stand-alone sampler's at the states they saw."""
    from revisit_bpr import engine as eng, native
    from revisit_bpr.foldin import fold_in

    fn = native.load().bpr_test_foldin_scored_plan
    fn.argtypes, fn.restype = [ctypes.POINTER(ctypes.c_int64)] * 2, ctypes.c_int
    out = (ctypes.c_int64 * 12)()
    I, d, K = 70_000, 32, 10
    lens = [0, 1, 3, 40, 300]
    assert fn((ctypes.c_int64 * 6)(len(lens), I, d, 0, 0, WARP if kind == "warp" else DYNAMIC), out) == 0
    assert (out[8], out[9], out[10]) == (0, 0, 0)  # bitmap, bm_words, lds_bytes
    rng = np.random.default_rng(70)
    rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)).astype(np.int32) for k in lens]
    indptr, items = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(rows).astype(np.int32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    Q[0] = 0
    P0 = (rng.standard_normal((len(lens), d)) * (4.0 / d ** 0.5)).astype(np.float32)
    gQ, gi, gp = gpu(Q), gpu(indptr), gpu(items)
    kw = dict(epochs=1, lr=LR, reg_user=0.01, init=gpu(P0), seed=SEED, offset=OFFSET, sampler=kind, candidates=K,
              max_sampled=K, margin=MARGIN, return_neg=True, return_draws=True)
    P, neg, tries, states = fold_in(gQ, None, gi, gp, _states=True, **kw)
    assert same(fold_in(gQ, None, gi, gp, _seen_mode=1, **kw), (P, neg, tries))
    assert same(fold_in(gQ, None, gi, gp, _seen_mode=2, **kw), (P, neg, tries))  # does not fit: not taken
    owner = np.repeat(np.arange(len(lens)), lens)
    e = eng.Engine(states.contiguous(), gQ.clone(), None, pad_user=None)
    e.bind_seen_csr(gpu(np.concatenate([[0], np.cumsum([lens[r] for r in owner])]).astype(np.int64)),
                    gpu(np.concatenate([rows[r] for r in owner]).astype(np.int32)))
    users = torch.arange(len(owner), dtype=torch.int32, device="cuda")
    if kind == "dynamic":
        want = (e.sample_dynamic(users, K, SEED, OFFSET), torch.zeros_like(neg))
    else:
        want = e.sample_warp(users, gp, K, SEED, OFFSET, margin=MARGIN)
    torch.cuda.synchronize()
    e.close()
    mismatch("negative", neg, want[0])
    mismatch("tries", tries, want[1])


# ---- 8. first, not best ------------------------------------------------------------------------------------------------
def test_warp_takes_the_first_violator_dynamic_the_best_and_nan_neither():
    from revisit_bpr.foldin import fold_in

    I, d, pos = 50, 8, 7
    off = next(o for o in range(1000) if len(set(dm.accepted(SEED, o, {pos}, I, 5))) == 5)
    a = dm.accepted(SEED, off, {pos}, I, 5)
    indptr, items = gpu(np.array([0, 1], np.int64)), gpu(np.array([pos], np.int32))
    p = np.zeros((1, d), np.float32)
    p[0, 0] = 1.0

    def run(kind, K, edit=()):
        Q = np.zeros((I, d), np.float32)
        Q[pos, 0], Q[a[1], 0], Q[a[4], 0] = 10.0, 9.5, 20.0  # margin 1: a_2 violates, a_5 scores higher, a_1 a_3 a_4 do not
        for item, v in edit:
            Q[item, 0] = v
        out = fold_in(gpu(Q), None, indptr, items, epochs=1, lr=0.0, init=gpu(p), seed=SEED, offset=off, sampler=kind,
                      candidates=K, max_sampled=K, margin=1.0, return_neg=True, return_draws=True)
        torch.cuda.synchronize()
        return int(out[1][0]), int(out[2][0])

    nan = float("nan")
    assert run("warp", 10) == (a[1], 2)
    assert run("dynamic", 5) == (a[4], 0)
    assert run("warp", 1) == (-1, 0)  # a_1 does not violate
    assert run("warp", 10, [(a[1], nan)]) == (a[4], 5)  # a NaN candidate never violates
    assert run("dynamic", 5, [(a[4], nan)]) == (a[1], 0)  # ... and never wins
    assert run("dynamic", 5, [(a[0], nan)]) == (a[4], 0)  # a NaN a_1 is replaced
    assert run("warp", 10, [(pos, nan)]) == (-1, 0)  # a NaN x_i: skipped


# ---- 9. nothing else is written ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_tables_csr_and_slack_are_never_written(kind, d):
    c = case(50, d)
    Q0, b0, P00, ip0, it0 = c.Q.clone(), c.b.clone(), c.P0.clone(), c.g_indptr.clone(), c.g_items.clone()
    pad, epochs = 64, 3
    for seen_mode in (0, 1, 2):
        bufs = raw(c, kind, 10, epochs=epochs, seen_mode=seen_mode, pad=pad)
        assert same(inner(bufs, c, epochs, pad), c.fold(kind, 10, epochs=epochs))
        assert bool((bufs[0][:pad] == -7.5).all()) and bool((bufs[0][-pad:] == -7.5).all())
        for o in bufs[1:]:
            assert bool((o[:pad] == -7).all()) and bool((o[-pad:] == -7).all())
    assert torch.equal(c.Q, Q0) and torch.equal(c.b, b0) and torch.equal(c.P0, P00)
    assert torch.equal(c.g_indptr, ip0) and torch.equal(c.g_items, it0)


# ---- 10. the surface ---------------------------------------------------------------------------------------------------
def make_rows(lens, I, rng):
    rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)).astype(np.int32) for k in lens]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(rows).astype(np.int32)


def test_engine_fold_in_is_the_free_function_and_adagrad_is_still_refused():
    from revisit_bpr import engine as eng, native
    from revisit_bpr.foldin import fold_in

    rng = np.random.default_rng(8)
    U, I, d = 500, 400, 64
    P = gpu(rng.normal(0, 0.1, (U, d)).astype(np.float32))
    Q = gpu(rng.normal(0, 0.5, (I, d)).astype(np.float32))
    b = gpu(rng.normal(0, 0.1, I).astype(np.float32))
    e = eng.Engine(P, Q, b)
    e.set_reg(0.02, 0.01, 0.01)
    e.set_optimizer(eng.OPT_SGD, lr=0.03)
    indptr, items = (gpu(x) for x in make_rows([0, 5, 30, 200, 12], I, rng))
    init = gpu(rng.normal(0, 0.5, (5, d)).astype(np.float32))
    kw = dict(epochs=4, seed=5, return_neg=True, init=init)
    uniform = e.fold_in(indptr, items, **kw)  # the default is the uniform path
    assert same(uniform, fold_in(e.Q, e.item_bias, indptr, items, lr=0.03, reg_user=0.02, **kw))
    for extra in (dict(sampler="dynamic", candidates=8), dict(sampler="warp", max_sampled=6, margin=0.5)):
        got = e.fold_in(indptr, items, return_draws=True, **extra, **kw)
        want = fold_in(e.Q.clone(), e.item_bias.clone(), indptr, items, lr=0.03, reg_user=0.02, return_draws=True,
                       **extra, **kw)
        assert same(got, want) and not torch.equal(got[1], uniform[1])
    # candidates = 1 under dynamic is the uniform sampler, bitwise
    assert same(e.fold_in(indptr, items, sampler="dynamic", candidates=1, **kw), uniform)
    lib = native.load()
    for kind in (DYNAMIC, WARP):  # the uniform entry point still refuses both kinds
        assert lib.bpr_fold_in_rows(1, None, 100, 8, 1, 1, 4, None, 3, 0.05, 0.0, kind, None, None, 0, 0, 1, None) == -3
    e.set_optimizer(eng.OPT_ADAGRAD, lr=0.03, eps=1e-10)
    for sampler in ("dynamic", "warp"):
        with pytest.raises(native.BprError) as ei:
            e.fold_in(indptr, items, sampler=sampler, **kw)
        assert ei.value.code == native.ERR_UNSUPPORTED and "Adagrad" in str(ei.value)


def test_model_fold_in_passes_the_sampler_through():
    from revisit_bpr.foldin import fold_in
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    U, I, d = 60, 300, 32
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"user": 0.03, "item": 0.001},
                logits_model=MF(torch.nn.Embedding(U, d, padding_idx=0), torch.nn.Embedding(I, d, padding_idx=0),
                                item_bias=True)).cuda()
    with torch.no_grad():
        model.logits_model._item_bias.copy_(torch.randn(I, device="cuda") * 0.1)
    indptr, items = (gpu(x) for x in make_rows([0, 4, 25, 120], I, np.random.default_rng(4)))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    Q, b = sd["logits_model._item_emb.weight"], sd["logits_model._item_bias"].reshape(-1)
    kw = dict(epochs=4, lr=0.05, seed=6, init_std=0.5)
    plain = fold_in(Q, b, indptr, items, reg_user=0.03, **kw)
    assert torch.equal(model.fold_in(indptr, items, **kw), plain)
    for extra in (dict(sampler="dynamic", candidates=8), dict(sampler="warp", max_sampled=6, margin=0.5)):
        got = model.fold_in(indptr, items, **extra, **kw)
        assert torch.equal(got, fold_in(Q, b, indptr, items, reg_user=0.03, **extra, **kw))
        assert not torch.equal(got, plain)
    for k, v in model.state_dict().items():  # the model itself is not changed
        assert torch.equal(v, sd[k]), k
