"""Item fold-in in both roles on the GPU: `bpr_fold_in_item_rows_roles`
(revisit-bpr_amd/csrc/bpr_foldin_items_roles.hip) and `fold_in_items(neg_role=...)` with what is built on it.

The reference is `restate` of tests/foldin_items_roles_model.py: the definition of include/bprcore.h step by step in
numpy (schedule, Philox draw, both updates).  Contract under test: with R = 0 the entry returns
`bpr_fold_in_item_rows`' bits; the training interaction of every negative-role step is the model's, exactly; the values
are the model's within the tolerance of tests/test_gpu_foldin_items.py (same comparison, same bound); the positive-role
draws do not depend on R; the result does not depend on `order`, `balance` or the other rows.

Shapes: U = 300, I = 60, 2 epochs, T = 2,000 training interactions (eight of them out of range), 7 rows with audiences
of 0, 1, 2, 5, 17, 64 and 298 (all but two) users; d = 8, 33, 96, 160, 300, 520: one per (G, E) class."""
import numpy as np
import pytest
import torch

from foldin_items_roles_model import restate
from test_gpu_foldin_items import BOUND, check_close, gpu, make_rows

pytestmark = pytest.mark.gpu

U0, I0, EPOCHS, LR, T0 = 300, 60, 2, 0.005, 2000
LENGTHS = [0, 1, 2, 5, 17, 64, 298]
M = len(LENGTHS)
DIMS = [8, 33, 96, 160, 300, 520]  # G = 32 with E = 1 / 2 / 4, G = 64 with E = 4 / 8 / 16
ROLES = [0, 1, 3, 40]
SEED, OFFSET = 11, 2 ** 32 + 1_000_003  # (a counter past 32 bits)

_rng = np.random.default_rng(21)
INDPTR, USERS, ROWS = make_rows(LENGTHS, U0, _rng)
NNZ = int(INDPTR[-1])
NEG = _rng.integers(1, I0, EPOCHS * NNZ).astype(np.int32)
NEG[[int(INDPTR[4]) + 4, int(INDPTR[6]) + 100, NNZ + int(INDPTR[5]) + 7]] = 0  # skipped triples
TRAIN_U = _rng.integers(0, U0, T0).astype(np.int32)
TRAIN_I = _rng.integers(1, I0, T0).astype(np.int32)
BAD_ENTRIES = [5, 400, 777, 1999, 13, 1200, 64, 1500]
TRAIN_U[BAD_ENTRIES[:4]] = [U0, -1, U0, -1]
TRAIN_I[BAD_ENTRIES[4:]] = [0, I0, 0, I0]
TRAIN = (TRAIN_U, TRAIN_I)
LEFT_OUT = np.setdiff1d(np.arange(U0), ROWS[6])  # the two users outside the last row's audience
_seen_lengths = list(_rng.integers(0, 12, U0))
_seen_lengths[7], _seen_lengths[9] = I0 - 1, I0 - 2  # a user who has seen every item, one who has seen all but one
SEEN_INDPTR, SEEN_INDICES, _ = make_rows(_seen_lengths, I0, _rng, first=1)


def tables(d):
    """Tables at the scale of a trained model (rows of norm ~ 0.1 sqrt(d)): the bound of
    tests/test_gpu_foldin_items.py was derived for fp32 rounding at values below 1."""
    rng = np.random.default_rng(300 + d)
    s = 0.5 / np.sqrt(d)
    P = rng.normal(0, s, (U0, d)).astype(np.float32)
    Q = rng.normal(0, s, (I0, d)).astype(np.float32)
    Q[0] = 0
    return dict(P=P, Q=Q, b=rng.normal(0, 0.2, I0).astype(np.float32), Q0=rng.normal(0, 0.1 * s, (M, d)).astype(np.float32),
                b0=rng.normal(0, 0.1, M).astype(np.float32))


def raw(T, bias, indptr, users, R, *, epochs=EPOCHS, reg=0.05, neg=None, order=None, seed=SEED, offset=OFFSET, seen=None,
        m=None, Q0=None, b0=None, indptr_at=0, neg_at=0, train=None, want_roles=True, status_only=False):
    """`bpr_fold_in_item_rows_roles` itself on device tensors (R None: `bpr_fold_in_item_rows`, the single-role entry,
    on the same arguments).  Returns (Q_new, bias_new, neg_out, role_out); buffers
    start at -7, so an entry that is not written shows.  `status_only`: the entry's return value, unchecked."""
    from revisit_bpr import native

    lib = native.load()
    U, (I, d) = T["P"].shape[0], T["Q"].shape
    m = indptr.numel() - 1 if m is None else m
    Qn = (T["Q0"] if Q0 is None else Q0).clone()
    bn = (T["b0"] if b0 is None else b0).clone() if bias else None
    ends = indptr[[indptr_at, indptr_at + m]].tolist()
    out = torch.full((epochs * (ends[1] - ends[0]),), -7, dtype=torch.int32, device="cuda") if neg is None else None
    roles = torch.full((epochs * m * R,), -7, dtype=torch.int32, device="cuda") if want_roles and R is not None else None
    tu, ti = (gpu(TRAIN_U), gpu(TRAIN_I)) if train is None else train
    shared = (T["P"].data_ptr(), U, T["Q"].data_ptr(), T["b"].data_ptr() if bias else None, I, d,
              None if seen is None else seen[0].data_ptr(), None if seen is None else seen[1].data_ptr(),
              indptr.data_ptr() + 8 * indptr_at, users.data_ptr(), m, None if order is None else order.data_ptr(), epochs,
              LR, reg, native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM,
              None if neg is None else neg.data_ptr() + 4 * neg_at,
              None if out is None or out.numel() == 0 else out.data_ptr(), seed, offset)
    ends = (Qn.data_ptr(), None if bn is None else bn.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if R is None:
        rc = lib.bpr_fold_in_item_rows(*shared, *ends)
    else:
        rc = lib.bpr_fold_in_item_rows_roles(*shared, tu.data_ptr(), ti.data_ptr(), tu.numel(), R,
                                             None if roles is None or roles.numel() == 0 else roles.data_ptr(), *ends)
    if status_only:
        return rc
    native.check(rc)
    torch.cuda.synchronize()
    return Qn, bn, out, roles


_MODEL = {}


def model(d, bias, R, neg, reg=0.05):
    """The definition's answer for the shared inputs (computed once per case, never changed).  `neg`: the given
    negatives, or the negatives the device drew (positive-role draws are bpr_sample_uniform's, held to the engine's
    by tests/test_gpu_foldin_items.py; here they must equal the single-role entry's)."""
    key = (d, bias, R, neg.tobytes(), reg)
    if key not in _MODEL:
        T = tables(d)
        _MODEL[key] = restate(T["P"], T["Q"], T["b"] if bias else None, INDPTR, USERS, neg, T["Q0"], T["b0"], EPOCHS, LR, reg,
                              R, TRAIN, SEED, OFFSET)
    return _MODEL[key]


def model_roles(R):
    """role_out of the definition: it does not depend on d, the bias or the negatives."""
    return model(8, False, R, NEG)[3]


# ---- 1. R = 0 is the single-role entry, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("d", DIMS)
def test_without_negative_role_steps_the_bits_are_the_single_role_entrys(d, sampled):
    T = {k: gpu(v) for k, v in tables(d).items()}
    bias = d != 33
    seen = (gpu(SEEN_INDPTR), gpu(SEEN_INDICES))
    kw = dict(neg=None if sampled else gpu(NEG), seed=SEED, offset=OFFSET, seen=seen if sampled else None)
    old = raw(T, bias, gpu(INDPTR), gpu(USERS), None, **kw)
    for train in (None, (torch.zeros(0, dtype=torch.int32, device="cuda"),) * 2):  # (R = 0 accepts NULL arrays)
        new = raw(T, bias, gpu(INDPTR), gpu(USERS), 0, train=train, **kw)
        assert torch.equal(new[0], old[0]) and (not bias or torch.equal(new[1], old[1]))
        assert not sampled or torch.equal(new[2], old[2])
    assert not torch.equal(old[0][1:], T["Q0"][1:])


# ---- 2. role_out, 3. values, 5. the positive-role sampler ------------------------------------------------------------
def test_the_committed_seed_hides_no_failure():
    """On the model: rows whose audience holds under half of the T interactions have no -1 at any R; the row that
    leaves two users out has some -1 and some hits; no entry is out of range or in the audience."""
    for R in ROLES[1:]:
        roles = model_roles(R).reshape(EPOCHS, M, R)
        for r in range(M):
            in_audience = np.isin(TRAIN_U, ROWS[r]).sum()
            taus = roles[:, r].ravel()
            if in_audience < T0 / 2:
                assert (taus >= 0).all(), (R, r)
            hit = taus[taus >= 0]
            assert not np.isin(TRAIN_U[hit], ROWS[r]).any() and not np.isin(hit, BAD_ENTRIES).any()
            assert ((TRAIN_U[hit] >= 0) & (TRAIN_U[hit] < U0) & (TRAIN_I[hit] >= 1) & (TRAIN_I[hit] < I0)).all()
    assert [int(np.isin(TRAIN_U, ROWS[r]).sum() < T0 / 2) for r in range(M)] == [1, 1, 1, 1, 1, 1, 0]
    last = model_roles(40).reshape(EPOCHS, M, 40)[:, 6]
    assert (last == -1).any() and (last >= 0).any()
    assert np.isin(TRAIN_U[last[last >= 0]], LEFT_OUT).all()


@pytest.mark.parametrize("R", ROLES[1:])
@pytest.mark.parametrize("d", DIMS)
def test_roles_values_and_positive_role_draws(d, R):
    """Given and sampled negatives, with and without a bias (alternating over the cases; every (d, R) runs both
    samplers).  Tolerance: BOUND of tests/test_gpu_foldin_items.py (4 x the fp32 rounding scale measured there,
    2.28e-06, against the float64 restatement), unchanged.  That scale, 5.70e-07, is a property of fp32 at the values
    its inputs reach; here the row of 298 users takes 596 + 2 R sequential steps and its bias grows by lr w at each, so
    lr is 0.005: with it the float32 restatement differs from the float64 one by at most 5.47e-07 over all 24 cases
    (`python tests/test_gpu_foldin_items_roles.py` prints each, on the CPU) — the scale the bound was derived from.
    (At lr 0.05 the figure is 3.06e-06 and at 0.01 1.06e-06: the bias of that row passes 4, where one fp32 ulp is
    already 4.8e-07.)  A step left out or applied twice moves an element by lr w |p| ~ 1e-04."""
    T = {k: gpu(v) for k, v in tables(d).items()}
    indptr, users = gpu(INDPTR), gpu(USERS)
    seen = (gpu(SEEN_INDPTR), gpu(SEEN_INDICES))
    want_roles = model_roles(R)
    for sampled in (False, True):
        bias = (DIMS.index(d) + ROLES.index(R) + sampled) % 2 == 0
        kw = dict(neg=None if sampled else gpu(NEG), seen=seen if sampled else None)
        q, b, neg, roles = raw(T, bias, indptr, users, R, **kw)
        roles = roles.cpu().numpy()
        assert np.array_equal(roles, want_roles)  # (2) exactly the model's interactions, -1 where it says so
        per_row = roles.reshape(EPOCHS, M, R)
        assert (per_row[:, :6] >= 0).all()  # no hidden failure in the rows with small audiences
        hit = roles[roles >= 0]
        assert not np.isin(hit, BAD_ENTRIES).any()
        for r in range(M):
            taus = per_row[:, r][per_row[:, r] >= 0]
            assert not np.isin(TRAIN_U[taus], ROWS[r]).any()
        if R == 40:
            assert (per_row[:, 6] == -1).any()
        if sampled:  # (5) the draws of the single-role entry, at every R
            old = raw(T, bias, indptr, users, None, seen=seen)
            assert torch.equal(neg, old[2]) and int(neg.min()) >= 0
            used = neg.cpu().numpy()
            users_of = np.tile(USERS, EPOCHS)
            assert (used[users_of == 7] == 0).all() and (users_of == 7).any()
        else:
            used = NEG
        want = model(d, bias, R, used)
        check_close(q, b, (want[0], want[1] if bias else None), f"d={d} R={R} sampled={sampled} bias={bias}")  # (3)
        assert not torch.equal(q[0], T["Q0"][0])  # the row without an audience learns from its second role


# ---- 4. independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, R", [(8, 3), (160, 40), (520, 1)])
def test_result_does_not_depend_on_order_balance_or_the_other_rows(d, R):
    """A row alone (m = 1, a slice of the CSR) has g = e R + rho where the full call has (e m + r) R + rho, and its
    positive-role counter starts at its own triple: with ONE epoch and GIVEN negatives both calls are lined up by
    offset + r R (sampled negatives would need a second, different shift of the same `offset`)."""
    from revisit_bpr.foldin_items import fold_in_items

    T = {k: gpu(v) for k, v in tables(d).items()}
    indptr, users = gpu(INDPTR), gpu(USERS)
    seen = (gpu(SEEN_INDPTR), gpu(SEEN_INDICES))
    tu, ti = gpu(TRAIN_U), gpu(TRAIN_I)
    rng = np.random.default_rng(3)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    for sampled in (False, True):
        kw = dict(neg=None if sampled else gpu(NEG), seen=seen if sampled else None)
        base = raw(T, True, indptr, users, R, **kw)
        base = base if sampled else (base[0], base[1], base[3])
        desc = gpu(np.argsort(-np.asarray(LENGTHS), kind="stable").astype(np.int32))
        perm = gpu(rng.permutation(M).astype(np.int32))
        for order in (None, desc, perm):
            again = raw(T, True, indptr, users, R, order=order, **kw)
            assert same(again if sampled else (again[0], again[1], again[3]), base)
        for balance in (True, False):
            w = fold_in_items(T["P"], T["Q"], T["b"], indptr, users, epochs=EPOCHS, lr=LR, reg_item=0.05, init=T["Q0"],
                              init_bias=T["b0"], neg=kw["neg"], seed=SEED, offset=OFFSET, balance=balance,
                              return_neg=sampled, seen_indptr=kw["seen"] and seen[0], seen_indices=kw["seen"] and seen[1],
                              neg_role=R, train_users=tu, train_items=ti, return_roles=True)
            assert same(w, base)
    full = raw(T, True, indptr, users, R, epochs=1, neg=gpu(NEG))
    for r in range(M):
        at = int(INDPTR[r])
        alone = raw(T, True, indptr, users, R, epochs=1, m=1, indptr_at=r, Q0=T["Q0"][r:r + 1], b0=T["b0"][r:r + 1],
                    neg=gpu(NEG), neg_at=at, offset=OFFSET + r * R)
        assert torch.equal(alone[0][0], full[0][r]) and torch.equal(alone[1][0], full[1][r]), r
        assert torch.equal(alone[3], full[3][r * R:(r + 1) * R])
    # an order entry of -1 or m is passed over: the row and its role_out entries are not touched
    holes = gpu(np.array([6, -1, 4, M, 2, 0, M, -1], np.int32))
    base = raw(T, True, indptr, users, R, neg=gpu(NEG))
    got = raw(T, True, indptr, users, R, neg=gpu(NEG), order=holes)
    roles, want = got[3].reshape(EPOCHS, M, R), base[3].reshape(EPOCHS, M, R)
    for r in range(M):
        keep = r in (6, 4, 2, 0)
        assert torch.equal(got[0][r], (base[0] if keep else T["Q0"])[r]) and got[1][r] == (base[1] if keep else T["b0"])[r]
        assert torch.equal(roles[:, r], want[:, r]) if keep else bool((roles[:, r] == -7).all())


def test_nothing_frozen_is_written():
    T = {k: gpu(v) for k, v in tables(96).items()}
    frozen = dict(P=T["P"], Q=T["Q"], b=T["b"], seen_indptr=gpu(SEEN_INDPTR), seen_indices=gpu(SEEN_INDICES),
                  indptr=gpu(INDPTR), users=gpu(USERS), tu=gpu(TRAIN_U), ti=gpu(TRAIN_I), Q0=T["Q0"], b0=T["b0"])
    before = {k: v.clone() for k, v in frozen.items()}
    raw(frozen, True, frozen["indptr"], frozen["users"], 40, seen=(frozen["seen_indptr"], frozen["seen_indices"]),
        train=(frozen["tu"], frozen["ti"]))
    for k, v in frozen.items():
        assert torch.equal(v, before[k]), k


# ---- 6. direction ----------------------------------------------------------------------------------------------------
def test_the_second_role_pushes_the_item_down_for_users_outside_its_audience():
    """generate_latent(400 users, 150 items, 12,000 actions, 8 factors), d = 32; 20 items held out, 10 epochs of STREAM
    training without them; both fold-ins 20 epochs, lr 0.05, reg_item 0.002, the same seed.  With s = <p_u, q_new> +
    b_new: the mean of s over (user outside the audience, new item) pairs with neg_role="auto" must be below the same
    mean with neg_role=0 (every negative-role step lowers s for its user: dq = -lr w p_u, db = -lr w, w > 0), and the
    mean over (audience user, new item) pairs must stay above the mean over pairs outside (the positive-role steps
    still raise it).
    Observed on the numpy model (401 x 151 tables, 131 warm items, T = 6,714, 1,041 interactions to fold in from,
    auto = 52; warm tables from a numpy SGD of the same length, since STREAM training needs the device): outside the
    audience +3.1321 with R = 0 against -0.4052 with auto; inside +4.2480 with R = 0, +1.6976 with auto; no step skipped.
    Observed on an MI355X: outside +3.1104 with R = 0 against -0.4545 with auto; inside +4.2782 and +1.7505."""
    from revisit_bpr import engine as eng
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.foldin_items import fold_in_items

    data = synthetic.generate_latent(400, 150, 12_000, factors=8, seed=5)
    U, I, d = data.num_users, data.num_items, 32
    rng = np.random.default_rng(6)
    cold = np.sort(rng.choice(np.arange(1, I), size=20, replace=False))
    new_id = np.zeros(I, np.int64)
    is_cold = np.zeros(I, bool)
    is_cold[cold] = True
    Iw = I - len(cold)
    new_id[~is_cold] = np.arange(Iw)
    new_id[cold] = Iw + np.arange(len(cold))
    tr_u, tr_i = data.users.astype(np.int64), new_id[data.items]
    warm = tr_i < Iw
    wu, wi = tr_u[warm], tr_i[warm]
    order = np.lexsort((wi, wu))
    wu, wi = wu[order].astype(np.int32), wi[order].astype(np.int32)
    w_indptr = np.concatenate([[0], np.cumsum(np.bincount(wu, minlength=U))]).astype(np.int64)
    cu, ci = tr_u[~warm], tr_i[~warm] - Iw
    order = np.lexsort((cu, ci))
    c_users = cu[order].astype(np.int32)
    c_indptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=len(cold)))]).astype(np.int64)
    g = torch.Generator(device="cuda").manual_seed(7)
    P = torch.randn(U, d, device="cuda", generator=g) * 0.1
    Q = torch.randn(Iw, d, device="cuda", generator=g) * 0.1
    P[0] = 0
    Q[0] = 0
    b = torch.zeros(Iw, device="cuda")
    e = eng.Engine(P, Q, b)
    e.set_reg(0.002, 0.002, 0.002)
    e.set_optimizer(eng.OPT_SGD, lr=0.05)
    e.bind_seen_csr(gpu(w_indptr), gpu(wi))
    e.set_stream_opts(True, 0)
    for ep in range(10):
        pu, pi = e.plan_epoch(gpu(wu), gpu(wi), len(wu), seed=7 + ep)
        e.train_stream(pu, pi, sampler=eng.NEG_UNIFORM, seed=7, offset=ep * len(wu))
    e.hot_fold()
    torch.cuda.synchronize()
    kw = dict(epochs=20, lr=0.05, reg_item=0.002, init_std=0.1, seed=8, seen_indptr=gpu(w_indptr), seen_indices=gpu(wi))
    got = {}
    for name, role in (("0", dict()), ("auto", dict(neg_role="auto", train_users=gpu(wu), train_items=gpu(wi)))):
        Qn, bn = fold_in_items(e.P, e.Q, e.item_bias, gpu(c_indptr), gpu(c_users), **kw, **role)
        s = (e.P.double() @ Qn.double().T + bn.double()).cpu().numpy()[1:]  # [U - 1, 20] (user 0 is the pad row)
        inside = np.zeros((U, len(cold)), bool)
        inside[c_users, np.repeat(np.arange(len(cold)), np.diff(c_indptr))] = True
        inside = inside[1:]
        got[name] = (s[~inside].mean(), s[inside].mean())
    e.close()
    print(f"mean score outside the audience: R = 0 {got['0'][0]:+.4f}, auto {got['auto'][0]:+.4f}; "
          f"inside: R = 0 {got['0'][1]:+.4f}, auto {got['auto'][1]:+.4f}")
    assert got["auto"][0] < got["0"][0]
    assert got["auto"][1] > got["auto"][0]


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def test_bad_role_arguments_are_refused_and_nothing_aborts():
    from revisit_bpr import native

    lib = native.load()
    T = {k: gpu(v) for k, v in tables(8).items()}
    indptr, users = gpu(INDPTR), gpu(USERS)
    tu, ti = gpu(TRAIN_U), gpu(TRAIN_I)
    none = (torch.zeros(0, dtype=torch.int32, device="cuda"),) * 2  # (data_ptr() of an empty tensor is NULL)
    invalid, unsupported = -1, -3  # BPR_ERR_INVALID, BPR_ERR_UNSUPPORTED
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    for kw, status, word in ((dict(R=-1), invalid, b"neg_role"),
                             (dict(R=2, train=(none[0], ti)), invalid, b"train_users"),
                             (dict(R=2, train=(tu, none[0])), invalid, b"train_items"),
                             (dict(R=2, train=(one[:0], ti)), invalid, b"train_users"),  # T = 0 (and so no array)
                             (dict(R=2 ** 28), unsupported, b"epochs * m * neg_role"),  # 2 * 7 * 2^28 >= 2^31
                             (dict(R=2 ** 27, epochs=2 ** 4), unsupported, b"epochs * m * neg_role")):
        kw = dict(kw)
        assert raw(T, True, indptr, users, kw.pop("R"), neg=gpu(NEG), want_roles=False, status_only=True, **kw) == status
        assert word in lib.bpr_last_error() and b"bpr_fold_in_item_rows_roles" in lib.bpr_last_error()
    with pytest.raises(native.BprError):
        raw(T, True, indptr, users, -3, neg=gpu(NEG), want_roles=False)
    q, _, _, roles = raw(T, True, indptr, users, 1, neg=gpu(NEG))  # the process goes on
    assert np.array_equal(roles.cpu().numpy(), model_roles(1)) and bool(torch.isfinite(q).all())


# ---- 8. Engine.fold_in_items, Model.fold_in_items --------------------------------------------------------------------
def test_engine_and_model_pass_the_second_role_through():
    from revisit_bpr import engine as eng
    from revisit_bpr.foldin_items import fold_in_items
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF, ItemKNN

    tu, ti = gpu(TRAIN_U), gpu(TRAIN_I)
    indptr, users = gpu(INDPTR), gpu(USERS)
    T = {k: gpu(v) for k, v in tables(33).items()}
    e = eng.Engine(T["P"].clone(), T["Q"].clone(), T["b"].clone())
    e.set_reg(0.02, 0.01, 0.01)
    e.set_optimizer(eng.OPT_SGD, lr=0.03)
    e.bind_seen_csr(gpu(SEEN_INDPTR), gpu(SEEN_INDICES))
    role = dict(neg_role=3, train_users=tu, train_items=ti, return_roles=True)
    got = e.fold_in_items(indptr, users, epochs=2, seed=5, **role)
    want = fold_in_items(T["P"], T["Q"], T["b"], indptr, users, epochs=2, lr=0.03, reg_item=0.01, seed=5,
                         seen_indptr=gpu(SEEN_INDPTR), seen_indices=gpu(SEEN_INDICES), **role)
    assert len(got) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))
    plain = e.fold_in_items(indptr, users, epochs=2, seed=5)
    assert not torch.equal(plain[0], got[0])
    auto = e.fold_in_items(indptr, users, epochs=2, seed=5, **dict(role, neg_role="auto"))
    assert auto[2].numel() == 2 * M * max(1, round(T0 / (I0 - 1)))
    e.close()

    U, I, d = U0, I0, 32
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"user": 0.03, "item": 0.004},
                logits_model=MF(torch.nn.Embedding(U, d, padding_idx=0), torch.nn.Embedding(I, d, padding_idx=0),
                                item_bias=True)).cuda()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    P, Q = sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"]
    b = sd["logits_model._item_bias"].reshape(-1)
    kw = dict(epochs=2, lr=0.05, seed=6, init_std=0.1, **role)
    got = model.fold_in_items(indptr, users, **kw)
    theirs = model.engine().fold_in_items(indptr, users, reg_item=0.004, **kw)
    free = fold_in_items(P, Q, b, indptr, users, reg_item=0.004, **kw)
    assert all(torch.equal(got[k], theirs[k]) and torch.equal(got[k], free[k]) for k in (0, 1, 2))
    assert int(got[2].min()) >= -1 and int(got[2].max()) < T0
    for k, v in model.state_dict().items():  # the model itself is not changed
        assert torch.equal(v, sd[k]), k
    knn = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        knn.fold_in_items(gpu(np.array([0, 1], np.int64)), gpu(np.array([3], np.int32)), epochs=1, lr=0.05, **role)


if __name__ == "__main__":  # on the CPU: the rounding scale of the value test on these inputs, per case
    overall = 0.0
    for d_ in DIMS:
        for R_ in ROLES:
            T_ = tables(d_)
            args_ = (T_["P"], T_["Q"], T_["b"], INDPTR, USERS, NEG, T_["Q0"], T_["b0"], EPOCHS, LR, 0.05, R_, TRAIN, SEED,
                     OFFSET)
            a64, a32 = restate(*args_), restate(*args_, f=np.float32)
            worst = max(float(np.abs(a32[0].astype(np.float64) - a64[0]).max()),
                        float(np.abs(a32[1].astype(np.float64) - a64[1]).max()))
            overall = max(overall, worst)
            print(f"d = {d_} R = {R_}: max |float32 - float64| = {worst:.2e}")
    print(f"largest {overall:.2e}; bound of the GPU test {BOUND:.2e}")
