"""Adagrad on the fused training paths (STRICT and batched STREAM) against tests/adagrad_model.py, the row-sparse numpy
restatement of torch.optim.Adagrad that tests/test_adagrad_model_cpu.py holds to torch itself.

Tolerance: the one tests/test_gpu_parity.py applies to RMSprop against the oracle
(test_stateful_optimizers_long_horizon_vs_dense_oracle, its lines 263-264): close(got, want, 2e-5), i.e.
|got - want| <= 2e-5 * max(1, |want|).  RMSprop and Adagrad share the shape g / (sqrt(state) + eps).  Rows outside every
batch, and everything a refusal must not touch, are compared bit for bit.
"""
import numpy as np
import pytest

import adagrad_model as am

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_parity import close, dev, make_engine, maxerr  # noqa: E402

TOL = 2e-5  # tests/test_gpu_parity.py:263-264
REG = (0.0016, 0.0001, 0.00375)
U, I, B = 40, 30, 16
LR, EPS = 0.05, 1e-10
ADAGRAD = 4


def problem(d, bias, seed):
    rng = np.random.default_rng(seed)
    P = ((rng.random((U, d)) - 0.5) * 0.4).astype(np.float32)  # (not shrunk with d: every width really moves)
    Q = ((rng.random((I, d)) - 0.5) * 0.4).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b = np.linspace(-0.1, 0.1, I).astype(np.float32) if bias else None
    return P, Q, b


def triples(steps, seed, n_users=U - 6, n_items=I - 5):
    """`steps` batches of B with users and items repeated inside a batch, the pad user and the pad item present, and
    the last users / items never drawn (rows outside every batch)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(1, n_users, steps * B).astype(np.int32)
    i = rng.integers(1, n_items, steps * B).astype(np.int32)
    j = rng.integers(1, n_items, steps * B).astype(np.int32)
    for s in range(steps):
        o = s * B
        u[o + 1] = u[o + 2] = u[o]  # a user three times
        i[o + 4] = i[o + 3]         # a positive twice
        j[o + 6] = i[o + 5]         # one triple's negative is another's positive
        u[o + 7] = 0                # the pad user
        i[o + 8] = 0                # the pad item as a positive
    j = np.where(j == i, j % (n_items - 1) + 1, j).astype(np.int32)
    return u, i, j


def model_run(P, Q, b, u, i, j, iav, lr_decay=0.0, t0=0):
    """The model over consecutive batches of B; returns the tables, the sums and the rows that were touched."""
    P, Q, b = P.copy(), Q.copy(), None if b is None else b.copy()
    sums = am.new_sums(P, Q, b, iav)
    seen = [set(), set(), set()]
    for k, lo in enumerate(range(0, len(u), B)):
        sl = slice(lo, lo + B)
        rows = am.step(P, Q, b, sums, u[sl], i[sl], j[sl], LR, lr_decay, EPS, t0 + k + 1, REG, abi=True)
        for s, r in zip(seen, rows):
            s.update(int(x) for x in r)
    return P, Q, b, sums, seen


def adagrad_engine(P, Q, b, iav, lr_decay=0.0):
    from revisit_bpr import engine as eng

    assert eng.OPT_ADAGRAD == ADAGRAD
    e = make_engine(P, Q, b, REG)
    e.set_optimizer(eng.OPT_ADAGRAD, lr=LR, eps=EPS, lr_decay=lr_decay)
    st = e.alloc_opt_state()
    assert st["mP"] is None and st["mQ"] is None and st["mb"] is None and st["vP"] is not None
    assert (st["vb"] is not None) == (b is not None)
    for t in st.values():
        if t is not None:
            t.fill_(iav)
    return e, st


def check_against_model(e, st, want, start, what):
    Pm, Qm, bm, sums, seen = want
    P0, Q0, b0, iav = start
    got = {"P": e.P.cpu().numpy(), "Q": e.Q.cpu().numpy(), "sP": st["vP"].cpu().numpy(), "sQ": st["vQ"].cpu().numpy()}
    ref = {"P": Pm, "Q": Qm, "sP": sums["P"], "sQ": sums["Q"]}
    if bm is not None:
        got["b"], got["sb"] = e.item_bias.cpu().numpy(), st["vb"].cpu().numpy()
        ref["b"], ref["sb"] = bm, sums["b"]
    for k in ref:
        print(f"{what} {k}: max err {maxerr(got[k], ref[k]):.3g}")
        assert close(got[k], ref[k], TOL), (what, k, maxerr(got[k], ref[k]))
    assert np.abs(Pm - P0).max() > 0.01 and np.abs(Qm - Q0).max() > 0.01  # the tables really moved
    # rows outside every batch: bit-unchanged, weights and sums
    for k, sk, n, rows, w0 in (("P", "sP", U, seen[0], P0), ("Q", "sQ", I, seen[1], Q0)) + \
            ((("b", "sb", I, seen[2], b0),) if bm is not None else ()):
        rest = np.setdiff1d(np.arange(n), sorted(rows))
        assert rest.size >= 5
        assert np.array_equal(got[k][rest].view(np.int32), w0[rest].view(np.int32)), (what, k)
        assert np.array_equal(got[sk][rest], np.full_like(got[sk][rest], iav)), (what, sk)
    assert not got["P"][0].any() and not got["Q"][0].any()  # the pad embedding rows


# ---- 1. STRICT against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,iav", [(20, 0.0), (32, 0.5), (128, 0.0), (256, 0.5)])
@pytest.mark.parametrize("bias", [False, True])
def test_strict_steps_and_train_strict_follow_the_model(d, iav, bias):
    """Eight steps through Engine.step (forward_grad + apply) and the same triples through train_strict: element loads
    (d = 20), vector loads (32), G = 32 with E = 4 (128) and G = 64 (256), item_bias on and off, torch's default
    accumulator (0) and a non-zero one."""
    steps = 8
    P, Q, b = problem(d, bias, seed=d)
    u, i, j = triples(steps, seed=d + 1)
    want = model_run(P, Q, b, u, i, j, iav)
    e, st = adagrad_engine(P, Q, b, iav)
    for s in range(steps):
        sl = slice(s * B, (s + 1) * B)
        e.step(dev(u[sl]), dev(i[sl]), dev(j[sl]))
    assert e.step_count == steps
    check_against_model(e, st, want, (P, Q, b, iav), "step")
    e2, st2 = adagrad_engine(P, Q, b, iav)
    e2.train_strict(dev(u), dev(i), B, sampler=0, neg=dev(j))
    assert e2.step_count == steps
    check_against_model(e2, st2, want, (P, Q, b, iav), "train_strict")


# ---- 2. through the mirror -----------------------------------------------------------------------------------------------
def _mirror_batches(Um, Im, steps, seed):
    """Batches in which no row occurs more than twice per table: two fp32 atomic adds commute, so the fused run is
    reproducible bit for bit."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        pu, pi = rng.permutation(np.arange(1, Um)), rng.permutation(np.arange(1, Im))
        u, i, j = pu[:B].copy(), pi[:B].copy(), pi[B:2 * B].copy()
        u[1] = u[0]
        i[3] = i[2]
        j[5] = i[4]
        out.append({"user": torch.from_numpy(u).cuda(), "item": torch.from_numpy(i)[:, None].cuda(),
                    "neg": torch.from_numpy(j)[:, None].cuda()})
    return out


def _mirror(Um, Im, d, seed):
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    torch.manual_seed(seed)
    model = BPR(fuse_forward=True, reg_alphas={"user": REG[0], "item": REG[1], "neg": REG[2]},
                logits_model=MF(torch.nn.Embedding(Um, d, padding_idx=0), torch.nn.Embedding(Im, d, padding_idx=0),
                                item_bias=True)).cuda()
    with torch.no_grad():
        model.logits_model._item_bias.copy_(torch.linspace(-0.1, 0.1, Im))
    opt = torch.optim.Adagrad(model.parameters(), lr=LR, lr_decay=0.05, initial_accumulator_value=0.1)
    return model, opt


def _loop(model, opt, data):
    model.train()
    for bt in data:
        model(bt)["loss"].backward()
        opt.step()
        opt.zero_grad()
    model.eval()


def test_mirror_with_torch_optim_adagrad_and_checkpoint_resume():
    """BPR(MF(...)) with a stock torch.optim.Adagrad: the fused backend against set_backend("torch") over five steps
    (parameters and state["sum"] to the tolerance, state["step"] torch's); a state_dict taken after step 3 and loaded
    into a fresh model and optimizer reproduces steps 4-5 of the uninterrupted fused run bit for bit."""
    from revisit_bpr.models.bpr import set_backend

    Um, Im, d = 60, 80, 64
    data = _mirror_batches(Um, Im, 5, seed=4)
    runs = {}
    for backend in ("hip", "torch"):
        set_backend(backend)
        try:
            model, opt = _mirror(Um, Im, d, seed=11)
            _loop(model, opt, data)
            runs[backend] = (model, opt)
        finally:
            set_backend("hip")
    (mh, oh), (mt, ot) = runs["hip"], runs["torch"]
    for ph, pt in zip(mh.parameters(), mt.parameters()):
        assert close(ph.detach().cpu().numpy(), pt.detach().cpu().numpy(), TOL)
        sh, stt = oh.state[ph], ot.state[pt]
        assert set(sh) == set(stt) == {"sum", "step"}
        assert close(sh["sum"].cpu().numpy(), stt["sum"].cpu().numpy(), TOL)
        assert float(sh["step"]) == float(stt["step"]) == 5.0
        assert float((sh["sum"] - 0.1).min()) >= 0.0 and float(sh["sum"].max()) > 0.1
    # checkpoint after step 3 -> fresh model and optimizer -> steps 4-5
    first, opt1 = _mirror(Um, Im, d, seed=11)
    _loop(first, opt1, data[:3])
    ck_model = {k: v.detach().clone() for k, v in first.state_dict().items()}
    ck_opt = opt1.state_dict()
    second, opt2 = _mirror(Um, Im, d, seed=99)
    second.load_state_dict(ck_model)
    opt2.load_state_dict(ck_opt)
    _loop(second, opt2, data[3:])
    assert second.engine().step_count == 5
    for ph, p2 in zip(mh.parameters(), second.parameters()):
        assert torch.equal(ph.detach(), p2.detach())
        assert torch.equal(oh.state[ph]["sum"], opt2.state[p2]["sum"])
        assert float(opt2.state[p2]["step"]) == 5.0


# ---- 3. batched STREAM in the sequential limit --------------------------------------------------------------------------
def _alone_flags(u, Bv):
    """Per triple: does its user occur once in its virtual batch?  (What the launch's k_valone computes.)"""
    out = np.zeros(len(u), bool)
    for lo in range(0, len(u), Bv):
        blk = u[lo:lo + Bv]
        vals, cnt = np.unique(blk, return_counts=True)
        out[lo:lo + Bv] = np.isin(blk, vals[cnt == 1])
    return out


@pytest.mark.parametrize("Bv", [16, 64])
@pytest.mark.parametrize("d,bias", [(32, True), (128, False)])
@pytest.mark.parametrize("direct", [1, 0])
def test_batched_stream_sequential_limit_follows_the_model(Bv, d, bias, direct):
    """bpr_train_stream_batched with max_inflight = 1 — by the header's own statement the reference's mini-batch loop —
    over four batches in two launches.  With B >= 16 the launch marks the users that occur once in their virtual batch
    (they step at once, under the row's lock: the r4 branch); the others park their gradient.  Both occur, from the
    inputs.  direct = 0 forces every row through the parked branch: the same result."""
    rng = np.random.default_rng(Bv + d)
    n = 4 * Bv
    u = rng.integers(1, U - 6, n).astype(np.int32)
    i = rng.integers(1, I - 5, n).astype(np.int32)
    j = rng.integers(1, I - 5, n).astype(np.int32)
    u[1] = u[0]
    u[Bv + 3] = u[Bv + 2]
    u[7], i[8] = 0, 0
    j = np.where(j == i, j % (I - 6) + 1, j).astype(np.int32)
    alone = _alone_flags(u, Bv)
    assert alone.any() and not alone.all()  # both branches of the user table
    P, Q, b = problem(d, bias, seed=d + Bv)
    iav = 0.0 if d == 32 else 0.5
    Pm, Qm, bm = P.copy(), Q.copy(), None if b is None else b.copy()
    sums = am.new_sums(Pm, Qm, bm, iav)
    seen = [set(), set(), set()]
    for k, lo in enumerate(range(0, n, Bv)):
        sl = slice(lo, lo + Bv)
        rows = am.step(Pm, Qm, bm, sums, u[sl], i[sl], j[sl], LR, 0.05, EPS, k + 1, REG, abi=True)
        for s, r in zip(seen, rows):
            s.update(int(x) for x in r)
    e, st = adagrad_engine(P, Q, b, iav, lr_decay=0.05)
    e.set_tuning("vs_direct", direct)
    cut = 2 * Bv
    e.train_stream_batched(dev(u[:cut]), dev(i[:cut]), Bv, sampler=0, neg=dev(j[:cut]), max_inflight=1)
    e.train_stream_batched(dev(u[cut:]), dev(i[cut:]), Bv, sampler=0, neg=dev(j[cut:]), max_inflight=1)
    e.flush_lazy()  # (closes the gradient steps still parked; nothing is replayed)
    assert e.step_count == 4
    check_against_model(e, st, (Pm, Qm, bm, sums, seen), (P, Q, b, iav), f"vstream B={Bv}")


# ---- 4. batched STREAM with the chip full ------------------------------------------------------------------------------
def test_batched_stream_full_chip_properties():
    """max_inflight = 0 on U = 2,000, I = 500, d = 64, one epoch of 20,000 triples in virtual batches of 256.  Staleness
    makes the bits run-dependent, so only properties: everything finite, every sum element >= its initial value, rows
    that never occur bit-unchanged, the epoch's mean BPR loss below the first batch's."""
    Uf, If, d, n, Bv, iav = 2000, 500, 64, 20000, 256, 0.1
    rng = np.random.default_rng(9)
    P = ((rng.random((Uf, d)) - 0.5) / d * 8).astype(np.float32)
    Q = ((rng.random((If, d)) - 0.5) / d * 8).astype(np.float32)
    P[0] = 0
    Q[0] = 0
    b = np.zeros(If, np.float32)
    u = rng.integers(1, Uf - 100, n).astype(np.int32)   # the last 100 users never occur
    i = rng.integers(1, 100, n).astype(np.int32)        # positives from a popular head ...
    j = rng.integers(100, If - 50, n).astype(np.int32)  # ... negatives from the tail; the last 50 items never occur
    e = make_engine(P, Q, b, REG)
    from revisit_bpr import engine as eng

    e.set_optimizer(eng.OPT_ADAGRAD, lr=LR, eps=EPS)
    st = e.alloc_opt_state()
    for t in st.values():
        if t is not None:
            t.fill_(iav)
    _, _, sc0 = e.forward(dev(u[:Bv]), dev(i[:Bv]), dev(j[:Bv]))
    first = float(sc0[0]) / Bv
    sc = torch.zeros(4, device="cuda")
    e.train_stream_batched(dev(u), dev(i), Bv, sampler=0, neg=dev(j), max_inflight=0, scalars=sc)
    e.flush_lazy()
    torch.cuda.synchronize()
    assert int(sc[3]) == n and e.step_count == (n + Bv - 1) // Bv
    mean = float(sc[0]) / n
    print(f"full chip: first batch loss {first:.4f}, epoch mean {mean:.4f}")
    assert mean < first
    for k, t in (("P", e.P), ("Q", e.Q), ("b", e.item_bias), ("sP", st["vP"]), ("sQ", st["vQ"]), ("sb", st["vb"])):
        assert bool(torch.isfinite(t).all()), k
    for k in ("vP", "vQ", "vb"):
        assert float(st[k].min()) >= np.float32(iav), k
    Pg, Qg, bg = e.P.cpu().numpy(), e.Q.cpu().numpy(), e.item_bias.cpu().numpy()
    assert np.array_equal(Pg[Uf - 100:], P[Uf - 100:]) and np.array_equal(Qg[If - 50:], Q[If - 50:])
    assert np.array_equal(bg[If - 50:], b[If - 50:])
    for k, lo in (("vP", Uf - 100), ("vQ", If - 50), ("vb", If - 50)):
        tail = st[k][lo:].cpu().numpy()
        assert np.array_equal(tail, np.full_like(tail, iav)), k
    assert np.abs(Pg[1:Uf - 100] - P[1:Uf - 100]).max() > 0.01


# ---- 5. no lazy work --------------------------------------------------------------------------------------------------------
def test_flush_lazy_has_nothing_to_do():
    """After five STRICT steps flush_lazy() and flush_items() leave all six tensors bit-identical.  (The Engine's timing
    counter covers the training launches only, not the flush kernels, so that no kernel is enqueued is read from the
    code — strict_flush_impl returns before its launches — and only the bit-identity is checked here.)"""
    d = 32
    P, Q, b = problem(d, True, seed=2)
    u, i, j = triples(5, seed=3)
    e, st = adagrad_engine(P, Q, b, 0.0)
    for s in range(5):
        sl = slice(s * B, (s + 1) * B)
        e.step(dev(u[sl]), dev(i[sl]), dev(j[sl]))
    torch.cuda.synchronize()
    tensors = (e.P, e.Q, e.item_bias, st["vP"], st["vQ"], st["vb"])
    before = [t.clone() for t in tensors]
    e.flush_lazy()
    e.flush_items()
    torch.cuda.synchronize()
    for t0, t1 in zip(before, tensors):
        assert torch.equal(t0.view(torch.int32), t1.view(torch.int32))
    assert e.step_count == 5


# ---- 6. lr_decay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["step", "train_strict"])
def test_lr_decay_counts_steps_from_one(path):
    """lr_decay = 0.05 over five steps against the model: clr_t = lr / (1 + (t - 1) * 0.05).  A 0-based t would make
    every step 5 % (relative) too long — thousands of tolerances."""
    d, steps, iav = 32, 5, 0.5
    P, Q, b = problem(d, True, seed=6)
    u, i, j = triples(steps, seed=7)
    want = model_run(P, Q, b, u, i, j, iav, lr_decay=0.05)
    off = model_run(P, Q, b, u, i, j, iav, lr_decay=0.05, t0=-1)  # the 0-based count: must be told apart
    assert not close(off[0], want[0], TOL)
    e, st = adagrad_engine(P, Q, b, iav, lr_decay=0.05)
    if path == "step":
        for s in range(steps):
            sl = slice(s * B, (s + 1) * B)
            e.step(dev(u[sl]), dev(i[sl]), dev(j[sl]))
    else:
        e.train_strict(dev(u[:2 * B]), dev(i[:2 * B]), B, sampler=0, neg=dev(j[:2 * B]))
        e.train_strict(dev(u[2 * B:]), dev(i[2 * B:]), B, sampler=0, neg=dev(j[2 * B:]))
    check_against_model(e, st, want, (P, Q, b, iav), f"lr_decay {path}")


# ---- 7. refusals on the device ------------------------------------------------------------------------------------------
def test_refusals_leave_the_tables_alone():
    """train_stream (the fused k_stream), the same with the LDS tier asked for, StreamTrainer and fold-in refuse the
    kind with the unsupported status; the tables and the sums are bit-identical afterwards."""
    from revisit_bpr import engine as eng
    from revisit_bpr import native
    from revisit_bpr.fast import StreamTrainer

    d = 32
    P, Q, b = problem(d, True, seed=8)
    u, i, j = triples(2, seed=9)
    e, st = adagrad_engine(P, Q, b, 0.25)
    tensors = (e.P, e.Q, e.item_bias, st["vP"], st["vQ"], st["vb"])
    before = [t.clone() for t in tensors]
    indptr = torch.arange(0, U + 1, dtype=torch.int64).cuda()
    indices = torch.arange(1, U + 1, dtype=torch.int32).cuda() % (I - 1) + 1
    e.bind_seen_csr(indptr, indices)

    def unchanged():
        torch.cuda.synchronize()
        return all(torch.equal(t0.view(torch.int32), t1.view(torch.int32)) for t0, t1 in zip(before, tensors))

    with pytest.raises(native.BprError) as ei:
        e.train_stream(dev(u), dev(i), sampler=eng.NEG_GIVEN, neg=dev(j))
    assert ei.value.code == native.ERR_UNSUPPORTED and "Adagrad" in str(ei.value) and unchanged()
    with pytest.raises(native.BprError) as ei:
        e.train_stream(dev(u), dev(i), sampler=eng.NEG_UNIFORM, seed=1)
    assert ei.value.code == native.ERR_UNSUPPORTED and unchanged()
    e.set_hot_lds(16, always=True)
    with pytest.raises(native.BprError) as ei:
        e.train_stream(dev(u), dev(i), sampler=eng.NEG_UNIFORM, seed=1)
    assert ei.value.code == native.ERR_UNSUPPORTED and unchanged()
    with pytest.raises(native.BprError) as ei:
        e.train_stream(dev(u), dev(i), sampler=eng.NEG_UNIFORM, seed=1, cut=True)
    assert ei.value.code == native.ERR_UNSUPPORTED and unchanged()
    e.set_hot_lds(0)
    hist_ptr = torch.tensor([0, 3], dtype=torch.int64).cuda()
    hist = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    with pytest.raises(native.BprError) as ei:
        e.fold_in(hist_ptr, hist, epochs=2, lr=0.05)
    assert ei.value.code == native.ERR_UNSUPPORTED and "plain SGD" in str(ei.value) and unchanged()
    with pytest.raises(native.BprError) as ei:
        e.fold_in_items(hist_ptr, hist, epochs=2, lr=0.05)
    assert ei.value.code == native.ERR_UNSUPPORTED and unchanged()
    # StreamTrainer is plain SGD on k_stream: handed an optimizer it names the trainer that runs it
    model, opt = _mirror(U, I, d, seed=1)
    w0 = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(NotImplementedError, match="BatchedStreamTrainer"):
        StreamTrainer(model, dev(u), dev(i), indptr, indices, lr=opt)
    assert all(torch.equal(a, p.detach()) for a, p in zip(w0, model.parameters()))
    # ... and the two trainers that carry stateful optimizers accept it
    from revisit_bpr.fast import BatchedStreamTrainer, StrictTrainer

    StrictTrainer(model, opt, dev(u), dev(i), indptr, indices, sampler="uniform", batch_size=B)
    BatchedStreamTrainer(model, opt, dev(u), dev(i), indptr, indices, sampler="uniform", batch_size=B)
