"""Fold-in with adaptive negatives on the GPU: `bpr_fold_in_rows_adaptive` (revisit-bpr_amd/csrc/bpr_foldin_adaptive.hip)
and what is built on it (revisit_bpr.foldin.fold_in(sampler="adaptive"), Engine.fold_in, Model.fold_in).

Nothing here restates the sampler or the update: the references are the library's own EXISTING entry points, and
every comparison is exact.  The negative of triple t must be what `Engine.sample_adaptive` draws for counter
offset + t for a user whose row is the folded row's state just before t (tests 1, 4); that state comes from the
existing `fold_in(neg=...)` on the row's prefixes, whose bits do not depend on n.  The update must be the existing
kernel's (test 2), epochs must chain (3), the result must be a pure function of its definition (5), nothing but
P_new and the three outputs may be written (6), the Engine / Model entry points must be the free function (7), and
the folded rows must rank held-out items (8)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, P_GEO, SEED, OFFSET = 0.05, 0.2, 11, 1_000_003
DIMS = [1, 8, 33, 128, 256]
ITEMS = [50, 300]  # 300: a walk takes 3 trips of 4 * 32 entries at G = 32, 2 of 4 * 64 at G = 64
PAD = 4


def lengths(I):
    return [0, 1, 2, 3, 9, 17, 40, I - 2, I - 1]  # I - 2: one item unseen; I - 1: none, every triple is skipped


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Case:
    """Tables, histories and the engine's snapshot of Q for one (I, d); built once, never changed."""

    def __init__(self, I, d):
        from revisit_bpr import engine as eng

        rng = np.random.default_rng(1000 * I + d)
        self.I, self.d, self.lens = I, d, lengths(I)
        self.rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)).astype(np.int32) for k in self.lens]
        self.indptr = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.items = np.concatenate(self.rows).astype(np.int32)
        self.n, self.nnz = len(self.lens), int(self.indptr[-1])
        Q = rng.normal(0, 0.5, (I, d)).astype(np.float32)
        Q[0] = 0
        self.Q, self.b = gpu(Q), gpu(rng.normal(0, 0.5, I).astype(np.float32))
        self.P0 = gpu(rng.normal(0, 0.1, (self.n, d)).astype(np.float32))
        self.g_indptr, self.g_items = gpu(self.indptr), gpu(self.items)
        self.engine = eng.Engine(torch.zeros(1, d, device="cuda"), self.Q.clone(), None, pad_user=None)
        self.engine.adaptive_refresh()
        self.order, self.sigma = self.engine.adaptive_snapshot()  # copies
        torch.cuda.synchronize()
        self.snapshot = (self.order, self.sigma)
        self.users_of = np.repeat(np.arange(self.n), self.lens).astype(np.int32)  # row of CSR position k

    def fold(self, epochs=1, bias=True, reg=0.05, lr=LR, init=None, offset=OFFSET, **kw):
        from revisit_bpr.foldin import fold_in

        out = fold_in(self.Q, self.b if bias else None, kw.pop("indptr", self.g_indptr), self.g_items, epochs=epochs,
                      lr=lr, reg_user=reg, init=self.P0 if init is None else init, seed=SEED, offset=offset,
                      sampler="adaptive", adaptive_p=P_GEO, snapshot=kw.pop("snapshot", self.snapshot),
                      return_neg=True, return_draws=True, **kw)
        torch.cuda.synchronize()
        return out

    def given(self, neg, epochs, bias=True, reg=0.05, init=None):
        from revisit_bpr.foldin import fold_in

        return fold_in(self.Q, self.b if bias else None, self.g_indptr, self.g_items, epochs=epochs, lr=LR,
                       reg_user=reg, init=self.P0 if init is None else init, neg=neg)

    def sampler_engine(self, P, indptr, indices):
        from revisit_bpr import engine as eng

        e = eng.Engine(P.contiguous(), self.Q.clone(), None, pad_user=None)
        e.bind_seen_csr(gpu(indptr), gpu(indices))
        e.adaptive_refresh()
        return e


_cases = {}


def case(I, d):
    if (I, d) not in _cases:
        _cases[(I, d)] = Case(I, d)
    return _cases[(I, d)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---- 1. the sampler is bpr_sample_adaptive's -------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_every_negative_is_the_engines_draw_for_the_row_as_it_stands(I, d, bias):
    from revisit_bpr.foldin import fold_in

    c = case(I, d)
    _, neg, fac, rnk = c.fold(epochs=1, bias=bias)
    neg_h = neg.cpu().numpy()
    # the state before the j-th triple of row r = the existing kernel's result on the row's first j positives with
    # the negatives this kernel used for them (epochs = 1: triple index = CSR position)
    pre_rows, pre_neg, owner = [], [], []
    for r in range(c.n):
        lo = int(c.indptr[r])
        for j in range(c.lens[r]):
            pre_rows.append(c.rows[r][:j])
            pre_neg.append(neg_h[lo:lo + j])
            owner.append(r)
    assert len(owner) == c.nnz
    pre_indptr = np.concatenate([[0], np.cumsum([len(x) for x in pre_rows])]).astype(np.int64)
    pre_items = np.concatenate(pre_rows + [np.zeros(0, np.int32)]).astype(np.int32)
    pre_negs = np.concatenate(pre_neg + [np.zeros(0, np.int32)]).astype(np.int32)
    states = fold_in(c.Q, c.b if bias else None, gpu(pre_indptr), gpu(pre_items), epochs=1, lr=LR, reg_user=0.05,
                     init=c.P0[gpu(np.asarray(owner, np.int64))], neg=gpu(pre_negs))
    # pseudo-user k: row = that state, seen = the WHOLE history of its row
    seen_indptr = np.concatenate([[0], np.cumsum([c.lens[r] for r in owner])]).astype(np.int64)
    seen = np.concatenate([c.rows[r] for r in owner]).astype(np.int32)
    e = c.sampler_engine(states, seen_indptr, seen)
    want = e.sample_adaptive(torch.arange(c.nnz, dtype=torch.int32, device="cuda"), P_GEO, SEED, OFFSET,
                             return_draws=True)
    torch.cuda.synchronize()
    for name, got, ref in zip(("negative", "factor", "rank"), (neg, fac, rnk), want):
        bad = torch.nonzero(got != ref).reshape(-1)
        assert bad.numel() == 0, (name, bad[:5].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())
    # the two rows whose answer is known without any sampler
    lo, hi = int(c.indptr[-3]), int(c.indptr[-2])
    only = np.setdiff1d(np.arange(1, I), c.rows[-2])
    assert len(only) == 1 and (neg_h[lo:hi] == only[0]).all()
    assert (neg_h[hi:] == 0).all()
    for r in range(c.n - 1):  # every other negative is an unseen item of its row
        for j in neg_h[c.indptr[r]:c.indptr[r + 1]]:
            assert 1 <= j < I and j not in c.rows[r]
    assert 0 <= int(fac.min()) and int(fac.max()) < d
    if d >= 8 and I == 50:
        assert len(np.unique(neg_h)) > 10 and len(np.unique(rnk.cpu().numpy())) > 5  # p = 0.2 spreads the ranks


# ---- 2. the update is the existing kernel's --------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_rows_are_the_given_negative_kernels_on_the_negatives_drawn(I, d, bias, reg):
    c = case(I, d)
    P, neg, _, _ = c.fold(epochs=3, bias=bias, reg=reg)
    assert neg.shape == (3 * c.nnz,)
    assert torch.equal(P, c.given(neg, 3, bias=bias, reg=reg))
    assert torch.equal(P[0], c.P0[0]) and torch.equal(P[-1], c.P0[-1])  # no triple; every triple skipped
    assert all(not torch.equal(P[r], c.P0[r]) for r in range(1, c.n - 1))


# ---- 3. epochs chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_three_epochs_are_three_calls_of_one(I, d):
    c = case(I, d)
    P, neg, fac, rnk = c.fold(epochs=3)
    Pe, parts = c.P0, []
    for e in range(3):
        Pe, *draws = c.fold(epochs=1, init=Pe, offset=OFFSET + e * c.nnz)
        parts.append(draws)
    assert torch.equal(P, Pe)
    for k, whole in enumerate((neg, fac, rnk)):
        assert torch.equal(whole, torch.cat([part[k] for part in parts]))


# ---- 4. a frozen row: the counters across epochs ---------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_with_lr_zero_every_negative_is_the_engines_for_the_initial_row(I, d):
    c = case(I, d)
    epochs = 4
    P, neg, fac, rnk = c.fold(epochs=epochs, lr=0.0, reg=0.0)
    assert torch.equal(P, c.P0)
    e = c.sampler_engine(c.P0.clone(), c.indptr, c.items)
    want = e.sample_adaptive(gpu(np.tile(c.users_of, epochs)), P_GEO, SEED, OFFSET, return_draws=True)
    torch.cuda.synchronize()
    assert same((neg, fac, rnk), want)
    per_epoch = neg.reshape(epochs, c.nnz)
    assert not torch.equal(per_epoch[0], per_epoch[1])  # (different counters draw differently)


# ---- 5. a pure function ----------------------------------------------------------------------------------------------
def padded_copy(order, fill):
    buf = torch.full((order.numel() + 2 * PAD,), fill, dtype=torch.int32, device="cuda")
    buf[PAD:-PAD] = order.reshape(-1)
    return buf


def raw(c, order_ptr, sigma, row_order=None, epochs=3, seen_mode=0):
    """The entry point itself: any row_order, an order pointer of the caller's, the seen structure forced."""
    from revisit_bpr import native

    lib = native.load()
    fn = lib.bpr_test_fold_in_rows_adaptive
    fn.restype = ctypes.c_int
    fn.argtypes = native.SIGNATURES["bpr_fold_in_rows_adaptive"][1] + [ctypes.c_int32]
    P = c.P0.clone()
    outs = [torch.full((epochs * c.nnz,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    native.check(fn(c.Q.data_ptr(), c.b.data_ptr(), c.I, c.d, order_ptr, sigma.data_ptr(), c.g_indptr.data_ptr(),
                    c.g_items.data_ptr(), c.n, None if row_order is None else row_order.data_ptr(), epochs, LR, 0.05,
                    P_GEO, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), SEED, OFFSET, P.data_ptr(),
                    torch.cuda.current_stream().cuda_stream, seen_mode))
    torch.cuda.synchronize()
    return (P, *outs)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_result_does_not_depend_on_order_call_seen_structure_or_snapshot_copy(I, d):
    from revisit_bpr.foldin import _PaddedOrder, snapshot_of

    c = case(I, d)
    base = c.fold(epochs=3)
    assert int(base[1].min()) >= 0
    buf = padded_copy(c.order, 0)
    ptr = buf.data_ptr() + 4 * PAD
    rng = np.random.default_rng(3)
    desc = gpu(np.argsort(-np.asarray(c.lens), kind="stable").astype(np.int32))
    for row_order in (None, desc, gpu(rng.permutation(c.n).astype(np.int32))):
        for seen_mode in (0, 1, 2):
            got = raw(c, ptr, c.sigma, row_order, seen_mode=seen_mode)
            assert same(got, base), (row_order, seen_mode)
            assert int(got[1].min()) >= 0  # every entry written
    for seen_mode in (1, 2):
        assert same(c.fold(epochs=3, _seen_mode=seen_mode), base)
    for balance in (True, False):
        assert same(c.fold(epochs=3, balance=balance), base)
    # the engine's own snapshot buffer, no copy
    eo, es = c.engine._snapshot_views(back=False)
    assert same(c.fold(epochs=3, snapshot=(_PaddedOrder(eo), es)), base)
    # a snapshot built in torch EQUALS the engine's on these tie-free tables, order and sigma, bit for bit; so does
    # what it folds, handed over or built by the wrapper itself (snapshot=None)
    to, ts = snapshot_of(c.Q)
    assert torch.equal(to, c.order)
    assert torch.equal(ts, c.sigma), (ts - c.sigma).abs().max().item()
    assert same(c.fold(epochs=3, snapshot=(to, ts)), base)
    assert same(c.fold(epochs=3, snapshot=None), base)
    # rows handed over one at a time as CSR slices, the counter advanced to keep t (epochs = 1)
    whole = c.fold(epochs=1)
    for r in range(c.n):
        lo, hi = int(c.indptr[r]), int(c.indptr[r + 1])
        one = c.fold(epochs=1, indptr=c.g_indptr[r:r + 2], init=c.P0[r:r + 1], offset=OFFSET + lo)
        assert torch.equal(one[0][0], whole[0][r]), r
        assert all(torch.equal(one[k], whole[k][lo:hi]) for k in (1, 2, 3)), r


# ---- 6. nothing else is written --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("I", ITEMS)
def test_tables_snapshot_and_slack_are_never_written(I, d):
    from revisit_bpr.foldin import _PaddedOrder

    c = case(I, d)
    Q0, b0, P00, o0, s0 = c.Q.clone(), c.b.clone(), c.P0.clone(), c.order.clone(), c.sigma.clone()
    buf = padded_copy(c.order, 12345)  # (slack the walk reads and must mask: not even a valid item id at I = 50)
    buf0 = buf.clone()
    got = raw(c, buf.data_ptr() + 4 * PAD, c.sigma)
    assert same(got, c.fold(epochs=3))  # what the slack holds does not matter
    assert torch.equal(buf, buf0) and bool((buf[:PAD] == 12345).all()) and bool((buf[-PAD:] == 12345).all())
    eo, es = c.engine._snapshot_views(back=False)
    c.fold(epochs=3, snapshot=(_PaddedOrder(eo), es))
    for seen_mode in (1, 2):
        c.fold(epochs=3, _seen_mode=seen_mode)
    assert torch.equal(c.Q, Q0) and torch.equal(c.b, b0) and torch.equal(c.P0, P00)
    assert torch.equal(c.order, o0) and torch.equal(c.sigma, s0)
    after = c.engine.adaptive_snapshot()
    assert torch.equal(after[0], o0) and torch.equal(after[1], s0) and torch.equal(c.engine.Q, Q0)


# ---- 7. Engine.fold_in and Model.fold_in -----------------------------------------------------------------------------
def make_rows(lens, I, rng):
    rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)).astype(np.int32) for k in lens]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(rows).astype(np.int32)


def test_engine_fold_in_adaptive_is_the_free_function_on_its_refreshed_snapshot():
    from revisit_bpr import engine as eng
    from revisit_bpr.foldin import fold_in

    rng = np.random.default_rng(8)
    U, I, d, n = 500, 400, 64, 6000
    P = gpu(rng.normal(0, 0.1, (U, d)).astype(np.float32))
    Q = gpu(rng.normal(0, 0.1, (I, d)).astype(np.float32))
    b = gpu(rng.normal(0, 0.1, I).astype(np.float32))
    e = eng.Engine(P, Q, b)
    e.set_reg(0.02, 0.01, 0.01)
    e.set_optimizer(eng.OPT_SGD, lr=0.03)
    e.bind_seen_csr(gpu(np.zeros(U + 1, np.int64)), gpu(np.zeros(0, np.int32)))
    indptr, items = (gpu(x) for x in make_rows([0, 5, 30, 200, 12], I, rng))
    kw = dict(epochs=4, seed=5, return_neg=True)
    with pytest.raises(RuntimeError, match="snapshot"):
        e.fold_in(indptr, items, sampler="adaptive", refresh=False, **kw)
    uniform = e.fold_in(indptr, items, **kw)  # the default is the uniform path, bit for bit
    assert same(uniform, fold_in(e.Q, e.item_bias, indptr, items, lr=0.03, reg_user=0.02, **kw))
    e.adaptive_refresh()
    stale = e.adaptive_snapshot()
    users, pos, neg = (gpu(rng.integers(1, hi, n).astype(np.int32)) for hi in (U, I, I))
    e.train_stream(users, pos, sampler=eng.NEG_GIVEN, neg=neg)  # the item table moves on; the snapshot is now stale
    kept = e.fold_in(indptr, items, sampler="adaptive", adaptive_p=0.1, refresh=False, **kw)
    torch.cuda.synchronize()
    assert same(e.adaptive_snapshot(), stale)  # refresh=False draws from the snapshot as it is
    assert same(kept, fold_in(e.Q.clone(), e.item_bias.clone(), indptr, items, lr=0.03, reg_user=0.02,
                              sampler="adaptive", adaptive_p=0.1, snapshot=stale, **kw))
    got = e.fold_in(indptr, items, sampler="adaptive", adaptive_p=0.1, **kw)  # refresh=True
    torch.cuda.synchronize()
    fresh = e.adaptive_snapshot()
    assert not torch.equal(fresh[0], stale[0])
    want = fold_in(e.Q.clone(), e.item_bias.clone(), indptr, items, lr=0.03, reg_user=0.02, sampler="adaptive",
                   adaptive_p=0.1, snapshot=fresh, **kw)
    assert same(got, want) and not torch.equal(got[1], kept[1]) and not torch.equal(got[1], uniform[1])


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
    kw = dict(epochs=4, lr=0.05, seed=6, init_std=0.1)
    assert torch.equal(model.fold_in(indptr, items, **kw), fold_in(Q, b, indptr, items, reg_user=0.03, **kw))
    got = model.fold_in(indptr, items, sampler="adaptive", adaptive_p=0.05, **kw)
    snap = model.engine().adaptive_snapshot()
    assert torch.equal(got, model.engine().fold_in(indptr, items, reg_user=0.03, sampler="adaptive", adaptive_p=0.05,
                                                   refresh=False, **kw))
    assert torch.equal(got, fold_in(Q, b, indptr, items, reg_user=0.03, sampler="adaptive", adaptive_p=0.05,
                                    snapshot=snap, **kw))
    assert not torch.equal(got, fold_in(Q, b, indptr, items, reg_user=0.03, **kw))
    for k, v in model.state_dict().items():  # the model itself is not changed
        assert torch.equal(v, sd[k]), k


# ---- 8. sanity of the outcome ----------------------------------------------------------------------------------------
def train_without(users, items, indptr, indices, U, I, d, epochs, lr, reg, seed):
    """The training of tools/foldin_probe.py's strong-generalisation study: uniform-negative STREAM epochs, SGD."""
    from revisit_bpr import engine as eng

    g = torch.Generator(device="cuda").manual_seed(seed)
    P = torch.randn(U, d, device="cuda", generator=g) * 0.1
    Q = torch.randn(I, d, device="cuda", generator=g) * 0.1
    P[0] = 0
    Q[0] = 0
    e = eng.Engine(P, Q)
    e.set_reg(reg, reg, reg)
    e.set_optimizer(eng.OPT_SGD, lr=lr)
    e.bind_seen_csr(indptr, indices)
    e.set_stream_opts(True, 0)
    n = users.numel()
    for ep in range(epochs):
        pu, pi = e.plan_epoch(users, items, n, seed=seed + ep)
        e.train_stream(pu, pi, sampler=eng.NEG_UNIFORM, seed=seed, offset=ep * n)
    e.hot_fold()
    torch.cuda.synchronize()
    e.close()
    return Q


def test_adaptive_fold_in_ranks_held_out_items():
    """The strong-generalisation study of DESIGN 4.7 (tools/foldin_probe.py: generate_latent, 4,000 users, 1,500
    items, 240,000 actions, 400 users held out of 60 epochs of training, d = 32, lr 0.05, reg 0.002).  nDCG@100 of
    the held-out users on their held-out items, all in this run: (a) untrained rows N(0, 0.1^2), (b) those rows
    after 20 epochs of uniform fold-in, (c) after 20 epochs of adaptive fold-in.  Required: c >= a + (b - a) / 2 —
    a condition against a broken sampler (seen items, the pad, one item over and over), not a performance claim."""
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.evaluation import evaluate_topk
    from revisit_bpr.foldin import fold_in

    U0, I0, d, epochs, lr, reg = 4000, 1500, 32, 60, 0.05, 0.002
    data = synthetic.generate_latent(U0, I0, 240_000, factors=16, seed=5)
    held = np.sort(np.random.default_rng(6).choice(np.arange(1, data.num_users), size=U0 // 10, replace=False))
    is_held = np.zeros(data.num_users, bool)
    is_held[held] = True
    keep = ~is_held[data.users]
    cnt = np.diff(data.indptr) * ~is_held
    Qw = train_without(gpu(data.users[keep]), gpu(data.items[keep]),
                       gpu(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)), gpu(data.indices[keep]),
                       data.num_users, data.num_items, d, epochs, lr, reg, seed=7)
    h_indptr = np.concatenate([[0], np.cumsum(np.diff(data.indptr)[held])]).astype(np.int64)
    h_items = np.concatenate([data.indices[data.indptr[u]:data.indptr[u + 1]] for u in held]).astype(np.int32)
    pos = np.searchsorted(data.eval_users, held)
    assert np.array_equal(data.eval_users[pos], held)
    e_indptr = np.concatenate([[0], np.cumsum(np.diff(data.eval_indptr)[pos])]).astype(np.int64)
    e_items = np.concatenate([data.eval_items[data.eval_indptr[k]:data.eval_indptr[k + 1]] for k in pos]).astype(np.int32)
    rows = torch.arange(len(held), dtype=torch.int32, device="cuda")
    hi, ht, ei, et = gpu(h_indptr), gpu(h_items), gpu(e_indptr), gpu(e_items)

    def ndcg(P):
        return evaluate_topk(P, Qw, None, rows, ei, et, hi, ht, ks=(100,))["ndcg@100"]

    init = torch.randn(len(held), d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)) * 0.1
    kw = dict(epochs=20, lr=lr, reg_user=reg, init=init, seed=8)
    a = ndcg(init)
    b = ndcg(fold_in(Qw, None, hi, ht, **kw))
    c = ndcg(fold_in(Qw, None, hi, ht, sampler="adaptive", **kw))
    print(f"nDCG@100: untrained {a:.4f}, uniform 20 epochs {b:.4f}, adaptive 20 epochs {c:.4f}; "
          f"required at least {a + 0.5 * (b - a):.4f}")
    assert b > a
    assert c >= a + 0.5 * (b - a)
