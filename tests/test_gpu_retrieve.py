"""The deep retrieval kernel (`bpr_retrieve_rows`, revisit-bpr_amd/csrc/bpr_retrieve.hip) and what is built on it
(revisit_bpr.retrieve, Engine.retrieve, Model.retrieve) on the GPU.  Every comparison is exact equality of bits.

References, both independent of the new kernel:
  (a) `recommend(k)` for k <= 128 (k_topk);
  (b) `score_candidates` over the shared list arange(1, I) with the seen CSR (k_rerank: every pair's score in
      recommend's bits, -inf where ineligible), ordered by a stable descending torch.sort over ascending ids, cut to
      k, entries at -inf turned into (-1, -inf).
Shapes are the smallest at which the kernel can go wrong: k around the buffer sizes (cap = 256, 512, 1024, 2048), I
around k and cap, d on both load paths, n around the user tile."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TI = 128


def cap_of(k):
    cap = 1
    while cap < max(k + TI, 2 * k):
        cap *= 2
    return cap


def make_csr(U, I, rng, density=0.2):
    """Seen CSR over U users (int64 [U+1], int32 sorted per row, items 1 .. I-1): user 0 has seen nothing, user 1
    everything but (at most) 3 items, user 2 everything, the rest a random subset."""
    rows = []
    for u in range(U):
        if u == 0 or I < 2:
            rows.append(np.zeros(0, np.int32))
        elif u == 1:
            keep = rng.choice(np.arange(1, I), size=min(3, I - 1), replace=False)
            rows.append(np.setdiff1d(np.arange(1, I), keep).astype(np.int32))
        elif u == 2:
            rows.append(np.arange(1, I, dtype=np.int32))
        else:
            rows.append(np.flatnonzero(rng.random(I - 1) < density).astype(np.int32) + 1)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, indices


def user_list(U, n, rng):
    """n user ids with users 0, 1, 2 (where they fit) and repeats among them."""
    users = rng.integers(0, U, n).astype(np.int32)
    users[0] = 0
    if n > 3:
        users[1], users[2] = 1, 2
        users[n - 1] = users[n // 2]  # a repeat for sure
    return users


def gpu(x):
    return None if x is None else torch.from_numpy(x).cuda()


def run(P, Q, b, users, k, indptr=None, indices=None, item_slices=0):
    """retrieve on device tensors -> (items, scores) on the device, shapes and dtypes checked"""
    from revisit_bpr.retrieve import retrieve

    items, scores = retrieve(P, Q, b, users, k, indptr, indices, item_slices=item_slices)
    torch.cuda.synchronize()
    assert items.shape == scores.shape == (users.numel(), k)
    assert items.dtype == torch.int32 and scores.dtype == torch.float32
    return items, scores


def reference(P, Q, b, users, k, indptr=None, indices=None):
    """(b): every pair's score from k_rerank, a stable sort, the cut, the padding"""
    from revisit_bpr.rerank import score_candidates

    n, I = users.numel(), Q.shape[0]
    cand = torch.arange(1, I, dtype=torch.int32, device="cuda")
    s = score_candidates(P, Q, b, users, cand, None, indptr, indices)  # [n, I - 1]
    assert s.shape == (n, I - 1) and not torch.isnan(s).any()
    srt, idx = torch.sort(s, dim=1, descending=True, stable=True)  # ties: the earlier, smaller id first
    ids = cand[idx]
    items = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    scores = torch.full((n, k), float("-inf"), dtype=torch.float32, device="cuda")
    m = min(k, I - 1)
    scores[:, :m] = srt[:, :m]
    items[:, :m] = torch.where(torch.isneginf(srt[:, :m]), torch.full_like(ids[:, :m], -1), ids[:, :m])
    return items, scores


def same(got, want):
    """ids equal and score BITS equal"""
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


def check_against_recommend(got, P, Q, b, users, k, indptr, indices):
    """checks 1 and 2: retrieve(k) is recommend(k) for k <= 128; beyond, its first 128 columns are recommend(128)"""
    from revisit_bpr.recommend import recommend

    kk = min(k, 128)
    want = recommend(P, Q, b, users, kk, indptr, indices)
    assert same((got[0][:, :kk].contiguous(), got[1][:, :kk].contiguous()), want)


# ---- 1. the sweep ------------------------------------------------------------------------------------------------
# (k, I, d, n, bias, csr, tables): I = 2, k, k + 1, cap - 1, cap, cap + 1, 2 cap + TI + 1, 5000; d = 3, 130 (and 1, 33)
# take the element-load path; "int": integer tables, ties everywhere; "view": P and Q are views one float off 16 bytes
SWEEP = [
    (1, 2, 1, 1, False, False, "int"),
    (128, 128, 3, 63, True, True, "int"),
    (129, 130, 32, 64, True, True, "float"),
    (255, 511, 33, 65, False, True, "int"),
    (256, 512, 128, 130, True, False, "float"),
    (257, 1025, 130, 65, True, True, "float"),
    (129, 2 * 512 + TI + 1, 3, 130, False, True, "int"),
    (1000, 2 * 2048 + TI + 1, 32, 64, True, True, "int"),
    (1024, 5000, 128, 130, True, True, "float"),
    (1, 5000, 32, 63, False, True, "float"),
    (256, 5000, 128, 65, True, True, "view"),
    (1024, 1024, 32, 1, True, False, "float"),
]


@pytest.mark.parametrize("k, I, d, n, bias, csr, tables", SWEEP)
def test_equals_both_references(k, I, d, n, bias, csr, tables):
    assert cap_of(k) in (256, 512, 1024, 2048)
    rng = np.random.default_rng(k * 100_003 + I * 131 + d * 7 + n)
    U = 40
    if tables == "int":  # every partial sum is exact, scores tie all the time
        P = rng.integers(-3, 4, (U, d)).astype(np.float32)
        Q = rng.integers(-3, 4, (I, d)).astype(np.float32)
        b = rng.integers(-4, 5, I).astype(np.float32) if bias else None
    else:
        P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
        b = rng.standard_normal(I).astype(np.float32) if bias else None
    tP, tQ, tb = gpu(P), gpu(Q), gpu(b)
    if tables == "view":
        tP = torch.cat([tP.new_zeros(1), tP.reshape(-1)])[1:].view(U, d)
        tQ = torch.cat([tQ.new_zeros(1), tQ.reshape(-1)])[1:].view(I, d)
        assert tP.data_ptr() % 16 == 4 and tQ.data_ptr() % 16 == 4 and tP.is_contiguous() and d % 4 == 0
    indptr, indices = make_csr(U, I, rng) if csr else (None, None)
    tptr, tidx = gpu(indptr), gpu(indices)
    tu = gpu(user_list(U, n, rng))
    got = run(tP, tQ, tb, tu, k, tptr, tidx)
    want = reference(tP, tQ, tb, tu, k, tptr, tidx)
    if csr and n > 3 and I > 4:  # the padding is exercised: all but 3 seen, everything seen
        assert (want[0][1] >= 0).sum() == min(3, k) and (want[0][2] == -1).all()
    assert same(got, want)
    check_against_recommend(got, tP, tQ, tb, tu, k, tptr, tidx)


# ---- 2. adversarial tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [129, 1024])
def test_adversarial_tables(k):
    cap = cap_of(k)
    I, U, d, n = 2 * cap + TI + 1, 12, 4, 70
    rng = np.random.default_rng(k)
    indptr, indices = make_csr(U, I, rng, density=0.3)
    tptr, tidx = gpu(indptr), gpu(indices)
    users = user_list(U, n, rng)
    tu = gpu(users)
    P = np.zeros((U, d), np.float32)
    P[:, 0] = 1 + np.arange(U) % 3  # positive: the order of a user's scores is the order of Q[:, 0]
    tP = gpu(P)
    ids = torch.arange(1, k + 1, dtype=torch.int32, device="cuda")

    def table(col0):
        Q = np.zeros((I, d), np.float32)
        Q[:, 0] = col0
        return gpu(Q)

    # every score ties: ids 1 .. k in order; with the CSR, the unseen ones in order
    zero = table(0)
    got = run(tP, zero, None, tu, k)
    assert torch.equal(got[0], ids.expand(n, k)) and (got[1] == 0).all()
    got = run(tP, zero, None, tu, k, tptr, tidx)
    assert same(got, reference(tP, zero, None, tu, k, tptr, tidx))
    # users 0, 1, 2: seen nothing / all but 3 / everything
    assert (got[0][0] == ids).all() and (got[0][1] >= 0).sum() == 3 and (got[0][2] == -1).all()
    # every Q row twice: pairs of equal scores, the smaller id first
    half = rng.standard_normal(((I + 1) // 2, d)).astype(np.float32)
    dup = gpu(np.repeat(half, 2, axis=0)[:I].copy())
    rP = gpu(rng.standard_normal((U, d)).astype(np.float32))
    got = run(rP, dup, None, tu, k, tptr, tidx)
    assert same(got, reference(rP, dup, None, tu, k, tptr, tidx))
    free = run(rP, dup, None, tu, k)  # nothing seen: both of a pair come back adjacent (pairs are (2 j, 2 j + 1))
    assert same(free, reference(rP, dup, None, tu, k))
    it = free[0][0].cpu().numpy()
    pos = {int(i): j for j, i in enumerate(it)}
    assert all(pos[i + 1] == pos[i] + 1 for i in it[:-1] if i % 2 == 0 and i + 1 < I)
    # strictly increasing with id: every tile beats tau, every tile appends, compactions at their maximum
    up = table(np.arange(I))
    got = run(tP, up, None, tu, k)
    assert torch.equal(got[0], torch.arange(I - 1, I - 1 - k, -1, dtype=torch.int32, device="cuda").expand(n, k))
    got = run(tP, up, None, tu, k, tptr, tidx)
    assert same(got, reference(tP, up, None, tu, k, tptr, tidx))
    # strictly decreasing with id: nothing beats tau after the first compaction
    down = table(-np.arange(I))
    got = run(tP, down, None, tu, k)
    assert torch.equal(got[0], ids.expand(n, k))
    got = run(tP, down, None, tu, k, tptr, tidx)
    want = reference(tP, down, None, tu, k, tptr, tidx)
    assert same(got, want)
    # the padding: user 1 has 3 eligible items, user 2 none, user 0 has seen nothing
    assert (got[0][1, :3] >= 0).all() and (got[0][1, 3:] == -1).all() and torch.isneginf(got[1][1, 3:]).all()
    assert (got[0][2] == -1).all() and torch.isneginf(got[1][2]).all()
    assert torch.equal(got[0][0], ids)
    check_against_recommend(got, tP, down, None, tu, k, tptr, tidx)


# ---- 3. purity, bitwise ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def float_case():
    rng = np.random.default_rng(77)
    U, I, d = 200, 5000, 32
    P, Q = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
    b = rng.standard_normal(I).astype(np.float32)
    indptr, indices = make_csr(U, I, rng, density=0.05)
    users = user_list(U, 130, rng)
    t = tuple(gpu(x) for x in (P, Q, b, users, indptr, indices))
    full = {k: run(*t[:4], k, t[4], t[5]) for k in (129, 1000)}  # computed once, shared, never written
    return t + (full,)


@pytest.mark.parametrize("k", [129, 1000])
def test_alone_permuted_and_repeated_rows_are_the_same_rows(float_case, k):
    P, Q, b, users, indptr, indices, full = float_case
    items, scores = full[k]
    assert same((items, scores), reference(P, Q, b, users, k, indptr, indices))
    for r in (0, 1, 2, 63, 64, 65, 129):  # alone: one user tile, the library slices the items
        assert same(run(P, Q, b, users[r:r + 1], k, indptr, indices), (items[r:r + 1], scores[r:r + 1])), r
    perm = torch.from_numpy(np.random.default_rng(5).permutation(130)).cuda()
    assert same(run(P, Q, b, users[perm], k, indptr, indices), (items[perm], scores[perm]))
    rep = torch.cat([users[:7]] * 10)  # 70 rows, every user 10 times
    assert same(run(P, Q, b, rep, k, indptr, indices), (items[:7].repeat(10, 1), scores[:7].repeat(10, 1)))
    assert same(run(P, Q, b, users, k, indptr, indices), (items, scores))  # and the same call twice


@pytest.mark.parametrize("k", [129, 1000])
def test_item_slices_do_not_change_a_bit(float_case, k):
    from revisit_bpr.retrieve import slices

    P, Q, b, users, indptr, indices, full = float_case
    most = min(64, 8192 // k, 40)  # the cap for this k, and for 5000 items: 40 tiles
    assert slices(130, 5000, 32, k, 64) == most
    for s in (1, 2, 3, most, 64):
        assert same(run(P, Q, b, users, k, indptr, indices, item_slices=s), full[k]), s
        assert same(run(P, Q, b, users[:3], k, indptr, indices, item_slices=s), (full[k][0][:3], full[k][1][:3])), s


def test_the_largest_k_at_the_largest_slice_count(float_case):
    P, Q, b, users, indptr, indices, _ = float_case
    want = reference(P, Q, b, users, 1024, indptr, indices)
    for s in (1, 8):
        assert same(run(P, Q, b, users, 1024, indptr, indices, item_slices=s), want), s


# ---- 4. public layers --------------------------------------------------------------------------------------------
def test_engine_retrieve_is_retrieve_on_its_tables(float_case):
    from revisit_bpr.engine import Engine
    from revisit_bpr.retrieve import retrieve

    P, Q, b, users, indptr, indices, full = float_case
    e = Engine(P.clone(), Q.clone(), b.clone())
    none = e.retrieve(users, 300)  # no CSR bound: only item 0 is left out
    assert same(none, retrieve(P, Q, b, users, 300))
    e.bind_seen_csr(indptr, indices)
    assert same(e.retrieve(users, 1000), full[1000])
    assert same(e.retrieve(users, 1000, item_slices=2), full[1000])
    assert same(e.retrieve(users, 300, exclude_seen=False), none)
    assert (none[0] > 0).all()
    e.close()


def test_a_side_stream_gives_the_same_bits(float_case):
    P, Q, b, users, indptr, indices, full = float_case
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run(P, Q, b, users, 1000, indptr, indices)
        sliced = run(P, Q, b, users, 1000, indptr, indices, item_slices=3)
    side.synchronize()
    assert same(got, full[1000]) and same(sliced, full[1000])


@pytest.mark.parametrize("user_bias", [False, True])
def test_model_retrieve_agrees_and_adds_the_user_bias(user_bias):
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF
    from revisit_bpr.retrieve import retrieve

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"all": 0.001},
                logits_model=MF(torch.nn.Embedding(data.num_users, 32, padding_idx=0),
                                torch.nn.Embedding(data.num_items, 32, padding_idx=0),
                                item_bias=True, user_bias=user_bias)).cuda()
    if user_bias:
        with torch.no_grad():
            model.logits_model._user_bias.copy_(torch.randn(data.num_users, device="cuda"))
    tptr, tidx = gpu(data.indptr), gpu(data.indices)
    model.bind_seen_csr(tptr, tidx)
    users = torch.arange(0, data.num_users, dtype=torch.int32, device="cuda")
    k = 200  # of 300 items: rows end in padding
    for exclude in (True, False):
        sd = model.state_dict()
        it, sc = retrieve(sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"],
                          sd["logits_model._item_bias"], users, k, tptr if exclude else None,
                          tidx if exclude else None)
        if user_bias:
            sc = sc + sd["logits_model._user_bias"][users.long()].unsqueeze(1)
        assert same(model.retrieve(users, k, exclude_seen=exclude), (it, sc))
    # and the first 128 columns are Model.recommend's
    got, rec = model.retrieve(users, k), model.recommend(users, 128)
    assert same((got[0][:, :128].contiguous(), got[1][:, :128].contiguous()), rec)


def test_model_retrieve_needs_the_mf_scorer():
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import ItemKNN

    model = BPR(logits_model=ItemKNN(30, 8)).cuda()
    with pytest.raises(NotImplementedError):
        model.retrieve(torch.zeros(1, dtype=torch.int32, device="cuda"), 300)


def test_refusals_on_device_tensors():
    from revisit_bpr.retrieve import retrieve

    P, Q = torch.zeros(4, 8, device="cuda"), torch.zeros(6, 8, device="cuda")
    users = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="1024"):
        retrieve(P, Q, None, users, 1025)
    with pytest.raises(ValueError, match="out of range"):
        retrieve(P, Q, None, users + 4, 3)
    with pytest.raises(ValueError, match="float32"):
        retrieve(P.double(), Q, None, users, 3)
    with pytest.raises(ValueError, match="embedding dim"):
        retrieve(P, Q[:, :4], None, users, 3)
    it, sc = retrieve(P, Q, None, users[:0], 1024)  # no users: empty tensors, no launch
    assert it.shape == sc.shape == (0, 1024)
