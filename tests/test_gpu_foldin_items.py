"""Item fold-in on the GPU: `bpr_fold_in_item_rows` (revisit-bpr_amd/csrc/bpr_foldin_items.hip) and what is built on
it (revisit_bpr.foldin_items.fold_in_items, Engine.fold_in_items, Model.fold_in_items).

The reference of every value test is `restate` below: the definition in include/bprcore.h as a loop over triples in
numpy.  Contract under test: the triples of a row are applied in order against the frozen tables; a triple with
negative 0, a user outside [0, U) or a given negative outside [1, I) is skipped; sampled negatives are
`bpr_sample_uniform`'s for the triple's USER at counter offset + triple index; the result is a pure function of the
inputs (not of `order`, of the other rows, of the launch, of the call); P, Q, item_bias and the CSRs are never
written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U0, I0, EPOCHS, LR = 40, 50, 3, 0.05
LENGTHS = [0, 1, 2, 3, 9, 17, 33, 40]  # 40 = every user; 33 and 40 outlast any ring
DIMS = [1, 8, 33, 128, 256, 600]  # G = 32 with E = 1 / 1 / 2 / 4, G = 64 with E = 4 and E = 16
SEEN_LENGTHS = [0, 1, 17, 48, 49] + [3, 7, 11, 5, 9] * 7  # user 3: all but item 23; user 4: every item
U_ALL_BUT_23, U_ALL = 3, 4


def restate(P, Q, b, indptr, users, neg, Q0, b0, epochs, lr, reg, f=np.float64):
    """The definition, triple by triple, in the number format `f`.  float32: every operation rounds to fp32 and
    the dot product is a sequential chain (cumsum adds left to right).  Returns (Q_new, bias_new or None)."""
    P, Q, Qn = P.astype(f), Q.astype(f), Q0.astype(f).copy()
    b, bn = (None, None) if b is None else (b.astype(f), b0.astype(f).copy())
    lr, reg, one = f(np.float32(lr)), f(np.float32(reg)), f(1)
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    for r in range(len(indptr) - 1):
        q = Qn[r]
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                u, j = int(users[k]), int(neg[e * nnz + k - base])
                if j == 0 or not 0 <= u < len(P) or not 1 <= j < len(Q):
                    continue
                x = np.cumsum(P[u] * (q - Q[j]), dtype=f)[-1]
                if b is not None:
                    x = f(x + f(bn[r] - b[j]))
                w = f(one / f(one + np.exp(x)))
                q += f(-lr) * (f(-w) * P[u] + reg * q)
                if b is not None:
                    bn[r] = f(bn[r] + f(lr * w))
    return Qn, bn


def make_rows(lengths, n_ids, rng, first=0):
    rows = [np.sort(rng.choice(np.arange(first, n_ids), size=k, replace=False)).astype(np.int32) for k in lengths]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), rows


def tables(d, m=len(LENGTHS), U=U0, I=I0):
    rng = np.random.default_rng(100 + d)
    P = rng.normal(0, 0.5, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.5, (I, d)).astype(np.float32)
    Q[0] = 0
    return dict(P=P, Q=Q, b=rng.normal(0, 0.5, I).astype(np.float32), Q0=rng.normal(0, 0.1, (m, d)).astype(np.float32),
                b0=rng.normal(0, 0.1, m).astype(np.float32))


_rng = np.random.default_rng(7)
INDPTR, USERS, ROWS = make_rows(LENGTHS, U0, _rng)
NNZ = int(INDPTR[-1])
NEG = _rng.integers(1, I0, EPOCHS * NNZ).astype(np.int32)
# given negatives of 0 (skipped triples), in the rows of 17, 33 and 40 users: epoch 0 of all three, epochs 1 and 2 of the last
ZEROS = [int(INDPTR[5]) + 4, int(INDPTR[6]), int(INDPTR[7]) + 39, NNZ + int(INDPTR[7]) + 7, 2 * NNZ + int(INDPTR[7])]
NEG[ZEROS] = 0
_seen_rows = [np.setdiff1d(np.arange(1, I0), [23]).astype(np.int32) if k == 48 else
              np.sort(_rng.choice(np.arange(1, I0), size=k, replace=False)).astype(np.int32) for k in SEEN_LENGTHS]
SEEN_INDPTR = np.concatenate([[0], np.cumsum(SEEN_LENGTHS)]).astype(np.int64)
SEEN_INDICES = np.concatenate(_seen_rows).astype(np.int32)
USERS_OF = np.tile(USERS, EPOCHS)  # the user of triple t (indptr[0] = 0)

# Rounding scale: the largest |restate(float32) - restate(float64)| over every d, bias on / off and reg_item 0 / 0.05
# on the inputs above (rows and biases), measured on the CPU (`python tests/test_gpu_foldin_items.py` prints it per d);
# the kernel gets 4 x: the project's margin for a tree-shaped dot against a chain (tests/test_gpu_foldin.py).
SCALE = 5.70e-07
BOUND = 4 * SCALE


def gpu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def raw(T, bias, indptr, users, *, epochs=EPOCHS, reg=0.05, neg=None, order=None, seed=0, offset=0, seen=None,
        m=None, Q0=None, b0=None, indptr_at=0, neg_at=0):
    """`bpr_fold_in_item_rows` itself on device tensors (the wrapper always passes an order or none: here any list;
    `indptr_at` / `neg_at`: start the CSR / the negatives at that entry).  Returns (Q_new, bias_new, neg_out)."""
    from revisit_bpr import native

    lib = native.load()
    U, (I, d) = T["P"].shape[0], T["Q"].shape
    m = indptr.numel() - 1 if m is None else m
    Qn = (T["Q0"] if Q0 is None else Q0).clone()
    bn = (T["b0"] if b0 is None else b0).clone() if bias else None
    ends = indptr[[indptr_at, indptr_at + m]].tolist()
    out = torch.full((epochs * (ends[1] - ends[0]),), -7, dtype=torch.int32, device="cuda") if neg is None else None
    native.check(lib.bpr_fold_in_item_rows(
        T["P"].data_ptr(), U, T["Q"].data_ptr(), T["b"].data_ptr() if bias else None, I, d,
        None if seen is None else seen[0].data_ptr(), None if seen is None else seen[1].data_ptr(),
        indptr.data_ptr() + 8 * indptr_at, users.data_ptr(), m, None if order is None else order.data_ptr(), epochs, LR,
        reg, native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM,
        None if neg is None else neg.data_ptr() + 4 * neg_at, None if out is None else out.data_ptr(), seed, offset,
        Qn.data_ptr(), None if bn is None else bn.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return Qn, bn, out


def check_close(got_q, got_b, want, label):
    err = np.abs(got_q.cpu().numpy() - want[0]).max()
    if want[1] is not None:
        err = max(err, np.abs(got_b.cpu().numpy() - want[1]).max())
    print(f"{label}: max |kernel - float64| = {err:.3e}, bound {BOUND:.3e}")
    assert err <= BOUND


# ---- 1. exactness, given negatives ---------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d", DIMS)
def test_given_negatives_match_the_restatement(d, bias, reg):
    """U = 40, I = 50, rows of 0, 1, 2, 3, 9, 17, 33, 40 users, 3 epochs, lr 0.05.  Tolerance: the float32 restatement
    (sequential dot) differs from the float64 one on these inputs by at most 1.01e-07 (d = 1), 2.05e-07 (8), 4.95e-07
    (33), 5.70e-07 (128), 2.80e-07 (256), 3.27e-07 (600): the rounding scale is the largest, 5.70e-07.  The kernel's
    dot is a tree, not a chain, so it may differ from either by about that much: it is allowed 4 x the scale,
    2.28e-06, against float64.  Five of the given negatives are 0 (ZEROS): those triples are skipped."""
    from revisit_bpr.foldin_items import fold_in_items

    T = tables(d)
    b = T["b"] if bias else None
    want = restate(T["P"], T["Q"], b, INDPTR, USERS, NEG, T["Q0"], T["b0"], EPOCHS, LR, reg)
    got = fold_in_items(gpu(T["P"]), gpu(T["Q"]), gpu(b), gpu(INDPTR), gpu(USERS), epochs=EPOCHS, lr=LR, reg_item=reg,
                        init=gpu(T["Q0"]), init_bias=gpu(T["b0"]) if bias else None, neg=gpu(NEG))
    torch.cuda.synchronize()
    got_q, got_b = got if bias else (got, None)
    check_close(got_q, got_b, want, f"d={d} bias={bias} reg={reg}")
    got_q = got_q.cpu().numpy()
    assert np.array_equal(got_q[0], T["Q0"][0])  # the row of length 0, bit for bit
    assert all(not np.array_equal(got_q[r], T["Q0"][r]) for r in range(1, len(LENGTHS)))
    if bias:
        got_b = got_b.cpu().numpy()
        assert got_b[0] == T["b0"][0] and all(got_b[r] != T["b0"][r] for r in range(1, len(LENGTHS)))


# ---- 2. sampled negatives ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, bias, reg, with_seen", [(1, True, 0.05, True), (8, False, 0.0, True), (33, True, 0.0, True),
                                                     (128, True, 0.05, True), (256, False, 0.05, True),
                                                     (600, True, 0.05, True), (128, True, 0.05, False)])
def test_sampled_negatives_are_the_engines_draws(d, bias, reg, with_seen):
    from revisit_bpr import engine as eng
    from revisit_bpr.foldin_items import fold_in_items

    seed, offset = 11, 1_000_003
    T = tables(d)
    b = T["b"] if bias else None
    seen_indptr = SEEN_INDPTR if with_seen else np.zeros(U0 + 1, np.int64)
    seen_indices = SEEN_INDICES if with_seen else np.zeros(0, np.int32)
    out = fold_in_items(gpu(T["P"]), gpu(T["Q"]), gpu(b), gpu(INDPTR), gpu(USERS), epochs=EPOCHS, lr=LR, reg_item=reg,
                        init=gpu(T["Q0"]), init_bias=gpu(T["b0"]) if bias else None, seed=seed, offset=offset,
                        return_neg=True, seen_indptr=gpu(seen_indptr) if with_seen else None,
                        seen_indices=gpu(seen_indices) if with_seen else None)
    torch.cuda.synchronize()
    got_q, got_b, neg = out if bias else (out[0], None, out[1])
    neg = neg.cpu().numpy()
    assert neg.shape == (EPOCHS * NNZ,)
    e = eng.Engine(gpu(T["P"]), gpu(T["Q"]), None)
    e.bind_seen_csr(gpu(seen_indptr), gpu(seen_indices))
    theirs = e.sample_uniform(gpu(USERS_OF), seed, offset).cpu().numpy()
    assert np.array_equal(neg, theirs)
    for t, (u, j) in enumerate(zip(USERS_OF, neg)):
        row = seen_indices[seen_indptr[u]:seen_indptr[u + 1]]
        if len(row) == I0 - 1:
            assert j == 0, t  # nothing unseen: the triple is skipped
        else:
            assert 1 <= j < I0 and j not in row, (t, u, j)
        if with_seen and u == U_ALL_BUT_23:
            assert j == 23, t  # the one unseen item
    if with_seen:
        assert (USERS_OF == U_ALL).any() and (USERS_OF == U_ALL_BUT_23).any()
    want = restate(T["P"], T["Q"], b, INDPTR, USERS, neg, T["Q0"], T["b0"], EPOCHS, LR, reg)
    check_close(got_q, got_b, want, f"d={d} seen={with_seen}")


# ---- 3. purity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 128, 256])
@pytest.mark.parametrize("sampled", [False, True])
def test_result_does_not_depend_on_order_rows_or_call(d, sampled):
    from revisit_bpr.foldin_items import fold_in_items

    T = {k: gpu(v) for k, v in tables(d).items()}
    indptr, users = gpu(INDPTR), gpu(USERS)
    seen = (gpu(SEEN_INDPTR), gpu(SEEN_INDICES))
    rng = np.random.default_rng(3)
    m = len(LENGTHS)
    kw = dict(neg=None if sampled else gpu(NEG), seed=4, offset=77, seen=seen if sampled else None)

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (not sampled or torch.equal(a[2], b[2]))

    base = raw(T, True, indptr, users, **kw)
    desc = gpu(np.argsort(-np.asarray(LENGTHS), kind="stable").astype(np.int32))
    perm = gpu(rng.permutation(m).astype(np.int32))
    for order in (None, desc, perm):  # (None again: a second call)
        again = raw(T, True, indptr, users, order=order, **kw)
        assert same(again, base)
        if sampled:
            assert int(again[2].min()) >= 0  # every entry written
    for balance in (True, False):
        w = fold_in_items(T["P"], T["Q"], T["b"], indptr, users, epochs=EPOCHS, lr=LR, reg_item=0.05, init=T["Q0"],
                          init_bias=T["b0"], neg=kw["neg"], seed=4, offset=77, balance=balance, return_neg=True,
                          seen_indptr=kw["seen"] and seen[0], seen_indices=kw["seen"] and seen[1])
        assert same(w, base)
    # one epoch: a row computed alone from its slice of the CSR, at its own counter, is the row of the full call
    full = raw(T, True, indptr, users, epochs=1, **kw)
    for r in range(m):
        at = int(INDPTR[r])
        alone = raw(T, True, indptr, users, epochs=1, m=1, indptr_at=r, Q0=T["Q0"][r:r + 1], b0=T["b0"][r:r + 1],
                    neg=kw["neg"], neg_at=at, seed=4, offset=77 + at, seen=kw["seen"])
        assert torch.equal(alone[0][0], full[0][r]) and torch.equal(alone[1][0], full[1][r]), r
        if sampled:
            assert torch.equal(alone[2], full[2][at:at + LENGTHS[r]])
    # an order entry of -1 or m is passed over without touching any row
    holes = gpu(np.array([7, -1, 5, m, 3, 1, m, -1], np.int32))
    got = raw(T, True, indptr, users, order=holes, **kw)
    for r in range(m):
        keep = r in (7, 5, 3, 1)
        assert torch.equal(got[0][r], (base[0] if keep else T["Q0"])[r]) and got[1][r] == (base[1] if keep else T["b0"])[r]


# ---- 4. read-only --------------------------------------------------------------------------------------------------
def test_nothing_frozen_is_written():
    from revisit_bpr.foldin_items import fold_in_items

    T = {k: gpu(v) for k, v in tables(128).items()}
    frozen = dict(P=T["P"], Q=T["Q"], b=T["b"], seen_indptr=gpu(SEEN_INDPTR), seen_indices=gpu(SEEN_INDICES),
                  indptr=gpu(INDPTR), users=gpu(USERS), init=T["Q0"], init_bias=T["b0"])
    before = {k: v.clone() for k, v in frozen.items()}
    for neg in (None, gpu(NEG)):
        q, b = fold_in_items(frozen["P"], frozen["Q"], frozen["b"], frozen["indptr"], frozen["users"], epochs=EPOCHS,
                             lr=LR, reg_item=0.05, init=frozen["init"], init_bias=frozen["init_bias"], neg=neg, seed=2,
                             seen_indptr=frozen["seen_indptr"], seen_indices=frozen["seen_indices"])
        torch.cuda.synchronize()
        for k, v in frozen.items():
            assert torch.equal(v, before[k]), k
        assert torch.equal(q[0], T["Q0"][0]) and b[0] == T["b0"][0]  # the empty row
        assert not torch.equal(q[7], T["Q0"][7]) and b[7] != T["b0"][7]
    z = fold_in_items(T["P"], T["Q"], None, frozen["indptr"], frozen["users"], epochs=1, lr=LR)  # zeros: w = 1/2
    assert torch.equal(z[0], torch.zeros_like(z[0])) and bool(z[1].abs().sum() > 0)
    kw = dict(epochs=1, lr=0.0, init_std=0.1, seed=9)
    s = fold_in_items(T["P"], T["Q"], None, frozen["indptr"], frozen["users"], **kw)
    assert torch.equal(s, fold_in_items(T["P"], T["Q"], None, frozen["indptr"], frozen["users"], **kw))
    assert 0.05 < float(s.std()) < 0.2


# ---- 5. bad ids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 256])
def test_bad_ids_never_become_addresses(d):
    T = tables(d)
    bad_users, bad_neg = USERS.copy(), NEG.copy()
    ku = [int(INDPTR[4]) + 2, int(INDPTR[7]) + 11]  # CSR positions whose user is replaced: every epoch skips them
    bad_users[ku[0]], bad_users[ku[1]] = -1, U0
    tn = [int(INDPTR[5]) + 3, NNZ + int(INDPTR[6]) + 20]  # triples whose negative is replaced
    bad_neg[tn[0]], bad_neg[tn[1]] = I0, -5
    removed = NEG.copy()
    removed[tn] = 0
    for e in range(EPOCHS):
        removed[[e * NNZ + k for k in ku]] = 0
    want = restate(T["P"], T["Q"], T["b"], INDPTR, USERS, removed, T["Q0"], T["b0"], EPOCHS, LR, 0.05)
    G = {k: gpu(v) for k, v in T.items()}
    before = {k: v.clone() for k, v in G.items()}
    q, b, _ = raw(G, True, gpu(INDPTR), gpu(bad_users), neg=gpu(bad_neg))
    check_close(q, b, want, f"d={d} given")
    # sampled: the bad users' triples draw nothing (0) and are skipped
    q, b, neg = raw(G, True, gpu(INDPTR), gpu(bad_users), seed=5, seen=(gpu(SEEN_INDPTR), gpu(SEEN_INDICES)))
    neg = neg.cpu().numpy()
    bad_t = [e * NNZ + k for e in range(EPOCHS) for k in ku]
    assert (neg[bad_t] == 0).all()
    check_close(q, b, restate(T["P"], T["Q"], T["b"], INDPTR, bad_users, neg, T["Q0"], T["b0"], EPOCHS, LR, 0.05),
                f"d={d} sampled")
    for k, v in G.items():
        assert torch.equal(v, before[k]), k


# ---- 6. it learns, 7. the rows feed the rest -----------------------------------------------------------------------
def planted(d=16, per=20, I=60):
    """Two user clusters with orthogonal rows (A: users 1..per along e_0, B: the next `per` along e_1), random frozen
    items, and two new items: one only cluster A touched, one only cluster B touched."""
    rng = np.random.default_rng(12)
    P = np.zeros((1 + 2 * per, d), np.float32)
    P[1:1 + per, 0] = rng.uniform(0.8, 1.2, per)
    P[1 + per:, 1] = rng.uniform(0.8, 1.2, per)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    Q[0] = 0
    A, B = np.arange(1, 1 + per, dtype=np.int32), np.arange(1 + per, 1 + 2 * per, dtype=np.int32)
    return P, Q, A, B, np.array([0, per, 2 * per], np.int64), np.concatenate([A, B])


def test_fold_in_learns_which_cluster_an_item_belongs_to():
    from revisit_bpr.foldin_items import fold_in_items

    P, Q, A, B, indptr, users = planted()
    Q_new = fold_in_items(gpu(P), gpu(Q), None, gpu(indptr), gpu(users), epochs=10, lr=LR, seed=1).cpu().numpy()
    score = P.astype(np.float64) @ Q_new.astype(np.float64).T  # [U, 2]
    print("item of A: mean score A", score[A, 0].mean(), "B", score[B, 0].mean(), "; item of B: A", score[A, 1].mean(),
          "B", score[B, 1].mean())
    assert score[A, 0].mean() > score[B, 0].mean()
    assert score[B, 1].mean() > score[A, 1].mean()


def test_folded_rows_feed_recommend_and_rank_items():
    from revisit_bpr.foldin_items import fold_in_items
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.recommend import recommend

    P, Q, A, B, indptr, users = planted()
    I = Q.shape[0]
    gP, gQ, gb = gpu(P), gpu(Q), gpu(np.zeros(I, np.float32))
    Q_new, b_new = fold_in_items(gP, gQ, gb, gpu(indptr), gpu(users), epochs=10, lr=LR, seed=1)
    Q_all, b_all = torch.cat((gQ, Q_new)), torch.cat((gb, b_new))
    top, _ = recommend(gP, Q_all, b_all, gpu(A), 5)
    top = top.cpu().numpy()
    assert top.shape == (len(A), 5) and (top >= 1).all() and (top < I + 2).all()
    assert (top == I).any(axis=1).all()  # the item cluster A touched (id I) is among every A user's top 5
    tgt = gpu(np.full(len(A), I, np.int32))
    rank, _, score = rank_items(gP, Q_all, b_all, gpu(A), gpu(np.arange(len(A) + 1, dtype=np.int64)), tgt)
    assert int(rank.max()) < 5 and bool(torch.isfinite(score).all())


# ---- 8. Engine.fold_in_items, Model.fold_in_items ------------------------------------------------------------------
def test_engine_fold_in_items_reads_both_tables_whole():
    """An Adam engine after a few STRICT steps: rows the optimizer has not replayed yet sit in P and Q.
    Engine.fold_in_items flushes them before it reads, so it equals fold_in_items on clones of the flushed tables."""
    from revisit_bpr import engine as eng
    from revisit_bpr.foldin_items import fold_in_items

    rng = np.random.default_rng(8)
    U, I, d, B = 300, 200, 32, 64
    e = eng.Engine(gpu(rng.normal(0, 0.1, (U, d)).astype(np.float32)), gpu(rng.normal(0, 0.1, (I, d)).astype(np.float32)),
                   gpu(rng.normal(0, 0.1, I).astype(np.float32)))
    e.set_reg(0.02, 0.01, 0.01)
    e.set_optimizer(eng.OPT_ADAM, lr=0.03)
    e.alloc_opt_state()
    s_indptr, s_indices, _ = make_rows(list(rng.integers(0, 12, U)), I, rng, first=1)
    e.bind_seen_csr(gpu(s_indptr), gpu(s_indices))
    for _ in range(3):
        e.step(gpu(rng.integers(1, U, B).astype(np.int32)), gpu(rng.integers(1, I, B).astype(np.int32)),
               gpu(rng.integers(1, I, B).astype(np.int32)))
    torch.cuda.synchronize()
    P_lazy, Q_lazy = e.P.clone(), e.Q.clone()
    indptr, users, _ = make_rows([0, 5, 30, 200, 12], U, rng)
    indptr, users = gpu(indptr), gpu(users)
    got = e.fold_in_items(indptr, users, epochs=4, seed=5)  # lr, reg_item: the engine's
    torch.cuda.synchronize()
    assert not torch.equal(e.P, P_lazy) and not torch.equal(e.Q, Q_lazy)  # fold_in_items replayed them
    kw = dict(epochs=4, lr=0.03, reg_item=0.01, seed=5, seen_indptr=gpu(s_indptr), seen_indices=gpu(s_indices))
    want = fold_in_items(e.P.clone(), e.Q.clone(), e.item_bias.clone(), indptr, users, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    stale = fold_in_items(P_lazy, Q_lazy, e.item_bias, indptr, users, **kw)
    assert not torch.equal(got[0], stale[0])
    free = e.fold_in_items(indptr, users, epochs=4, seed=5, exclude_seen=False)
    want = fold_in_items(e.P, e.Q, e.item_bias, indptr, users, epochs=4, lr=0.03, reg_item=0.01, seed=5)
    assert torch.equal(free[0], want[0]) and not torch.equal(free[0], got[0])


def test_model_fold_in_items_is_the_engines_with_the_models_regularisation():
    from revisit_bpr.foldin_items import fold_in_items
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    U, I, d = 60, 300, 32
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"user": 0.03, "item": 0.004},
                logits_model=MF(torch.nn.Embedding(U, d, padding_idx=0), torch.nn.Embedding(I, d, padding_idx=0),
                                item_bias=True)).cuda()
    with torch.no_grad():
        model.logits_model._item_bias.copy_(torch.randn(I, device="cuda") * 0.1)
    indptr, users, _ = make_rows([0, 4, 25, 50], U, np.random.default_rng(4))
    indptr, users = gpu(indptr), gpu(users)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    P, Q = sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"]
    b = sd["logits_model._item_bias"].reshape(-1)
    kw = dict(epochs=4, lr=0.05, seed=6, init_std=0.1)
    got = model.fold_in_items(indptr, users, **kw)
    theirs = model.engine().fold_in_items(indptr, users, reg_item=0.004, **kw)
    free = fold_in_items(P, Q, b, indptr, users, reg_item=0.004, **kw)
    assert all(torch.equal(got[k], theirs[k]) and torch.equal(got[k], free[k]) for k in (0, 1))
    assert not torch.equal(got[0], fold_in_items(P, Q, b, indptr, users, reg_item=0.0, **kw)[0])
    other = model.fold_in_items(indptr, users, reg_item=0.0, **kw)  # an explicit value wins
    assert torch.equal(other[0], fold_in_items(P, Q, b, indptr, users, reg_item=0.0, **kw)[0])
    for k, v in model.state_dict().items():  # the model itself is not changed
        assert torch.equal(v, sd[k]), k


def test_model_fold_in_items_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        model.fold_in_items(gpu(np.array([0, 1], np.int64)), gpu(np.array([3], np.int32)), epochs=1, lr=0.05)


if __name__ == "__main__":  # the rounding scale of test 1, on the CPU
    overall = 0.0
    for d_ in DIMS:
        worst = 0.0
        for bias_ in (False, True):
            for reg_ in (0.0, 0.05):
                T_ = tables(d_)
                args_ = (T_["P"], T_["Q"], T_["b"] if bias_ else None, INDPTR, USERS, NEG, T_["Q0"], T_["b0"], EPOCHS, LR,
                         reg_)
                a64, a32 = restate(*args_), restate(*args_, np.float32)
                worst = max(worst, float(np.abs(a32[0].astype(np.float64) - a64[0]).max()))
                if bias_:
                    worst = max(worst, float(np.abs(a32[1].astype(np.float64) - a64[1]).max()))
        overall = max(overall, worst)
        print(f"d = {d_}: max |float32 - float64| = {worst:.2e}")
    print(f"SCALE = {overall:.2e}")
    P_, Q_, A_, B_, ip_, us_ = planted()
    ng_ = np.random.default_rng(0).integers(1, Q_.shape[0], 10 * len(us_))
    Qn_, _ = restate(P_, Q_, None, ip_, us_, ng_, np.zeros((2, 16), np.float32), None, 10, LR, 0.0)
    s_ = P_.astype(np.float64) @ Qn_.T
    print("planted (numpy, random negatives): item of A: A", s_[A_, 0].mean(), "B", s_[B_, 0].mean(), "; item of B: A",
          s_[A_, 1].mean(), "B", s_[B_, 1].mean())
