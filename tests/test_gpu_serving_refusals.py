"""The refusals of the serving wrappers that sit behind their device check — `recommend`, `retrieve`, `sample_items`,
`neighbors`, `diversify` — on tiny device tensors: the exception's type and its full message, and for two faults at
once which one is met.  No case launches a kernel except the last of each wrapper, which holds the `users` dtypes a
wrapper converts to the int32 call's result.  tests/test_serving_refusals_cpu.py has what CPU tensors reach."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U, I, D, N, K = 8, 16, 4, 3, 2


def raises(kind, message, fn, *args, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind
    assert str(e.value) == message


@pytest.fixture(scope="module")
def t():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    P, Q, b = torch.randn(U, D, generator=g), torch.randn(I, D, generator=g), torch.randn(I, generator=g)
    sptr = torch.tensor([0, 1, 1, 2, 2, 2, 2, 2, 3])
    sidx = torch.tensor([3, 5, 7], dtype=torch.int32)
    return dict(P=P.to(dev), Q=Q.to(dev), b=b.to(dev), users=torch.tensor([1, 2, 7], dtype=torch.int32, device=dev),
                sptr=sptr.to(dev), sidx=sidx.to(dev), dev=dev)


def wrappers():
    from revisit_bpr.recommend import recommend
    from revisit_bpr.retrieve import retrieve
    from revisit_bpr.sample import sample_items

    return [(recommend, "recommend"), (retrieve, "retrieve"), (sample_items, "sample_items")]


SHARE = "P [U, d] and Q [I, d] must share the embedding dim"
SEEN_T = "seen_indptr must be int64 and seen_indices int32"


@pytest.mark.parametrize("which", [0, 1, 2])
def test_user_wrappers_refuse_behind_the_device_check(t, which):
    fn, name = wrappers()[which]
    P, Q, b, users, sptr, sidx = t["P"], t["Q"], t["b"], t["users"], t["sptr"], t["sidx"]
    same = f"{name} needs every tensor on the device of P"
    rocm = f"{name} needs the tables and the user list on a ROCm device; there is no CPU path in libbprcore"
    for message, args in [
        ("P must be float32", (P.double(), Q, b, users, K)), ("Q must be float32", (P, Q.half(), b, users, K)),
        ("item_bias must be float32", (P, Q, b.double(), users, K)),
        (SHARE, (P, Q[:, :3], b, users, K)), (SHARE, (P[0], Q, b, users, K)), (SHARE, (P, Q[0], b, users, K)),
        ("item_bias must have one entry per item row", (P, Q, b[:5], users, K)),
        ("seen_indptr and seen_indices go together", (P, Q, b, users, K, sptr)),
        ("seen_indptr and seen_indices go together", (P, Q, b, users, K, None, sidx)),
        (SEEN_T, (P, Q, b, users, K, sptr.int(), sidx)), (SEEN_T, (P, Q, b, users, K, sptr, sidx.long())),
        ("seen_indptr must have U+1 entries", (P, Q, b, users, K, sptr[:8], sidx)),
        ("user id out of range", (P, Q, b, torch.tensor([1, U], dtype=torch.int32, device=t["dev"]), K)),
        ("user id out of range", (P, Q, b, torch.tensor([-1, 2], dtype=torch.int32, device=t["dev"]), K)),
        # two at once, in the wrappers' order: tables, shapes, bias, (users, draw_ids,) the seen CSR, the ids
        ("P must be float32", (P.double(), Q[:, :3], b, users, K)),
        ("Q must be float32", (P, Q.double(), b[:5], users, K)),
        (SHARE, (P, Q[:, :3], b[:5], users, K)),
        ("item_bias must have one entry per item row", (P, Q, b[:5], users, K, sptr)),
        ("seen_indptr and seen_indices go together",
         (P, Q, b, torch.tensor([U], dtype=torch.int32, device=t["dev"]), K, sptr)),
        (SEEN_T, (P, Q, b, users, K, sptr[:8].int(), sidx)),
    ]:
        raises(ValueError, message, fn, *args)
    # a tensor on the CPU among device tensors
    raises(RuntimeError, rocm, fn, P, Q.cpu(), b, users, K)
    raises(RuntimeError, rocm, fn, P, Q, b.cpu(), users, K)
    raises(RuntimeError, rocm, fn, P, Q, b, users.cpu(), K)
    raises(RuntimeError, same, fn, P, Q, b, users, K, sptr.cpu(), sidx)
    raises(RuntimeError, same, fn, P, Q, b, users, K, sptr, sidx.cpu())
    raises(RuntimeError, same, fn, P.double(), Q, b, users, K, sptr.cpu(), sidx)  # the device before the dtype
    raises(ValueError, "k must be at least 1", fn, P, Q.cpu(), b, users, 0)  # k before the device


def test_users_dtype_is_where_the_user_wrappers_differ(t):
    from revisit_bpr.recommend import recommend
    from revisit_bpr.retrieve import retrieve
    from revisit_bpr.sample import sample_items

    P, Q, b, users, sptr, sidx = t["P"], t["Q"], t["b"], t["users"], t["sptr"], t["sidx"]
    raises(ValueError, "users must be int32 or int64", sample_items, P, Q, b, users.double(), K)
    raises(ValueError, "users must be int32 or int64", sample_items, P, Q, b, users.double(), K, sptr)  # before the CSR
    raises(ValueError, "item_bias must have one entry per item row", sample_items, P, Q, b[:5], users.double(), K)
    for fn in (recommend, retrieve, sample_items):
        want = fn(P, Q, b, users, K, sptr, sidx)
        kinds = (torch.int64,) if fn is sample_items else (torch.int64, torch.float64)
        for kind in kinds:  # (the ids are whole numbers: the conversion is exact)
            got = fn(P, Q, b, users.to(kind).reshape(1, N), K, sptr, sidx)
            assert all(torch.equal(a, c) for a, c in zip(got, want))
        assert want[0].shape == (N, K) and want[0].dtype == torch.int32
        assert int(want[0].min()) >= 1  # (I - 1 - seen >= K eligible items: no padding)


def test_sample_items_draw_ids(t):
    from revisit_bpr.sample import sample_items

    P, Q, b, users, sptr = t["P"], t["Q"], t["b"], t["users"], t["sptr"]
    ids = torch.arange(N, device=t["dev"])
    raises(ValueError, "draw_ids must be int64", sample_items, P, Q, b, users, K, draw_ids=ids.int())
    raises(ValueError, "draw_ids must have one entry per row of users", sample_items, P, Q, b, users, K,
           draw_ids=ids[:2])
    raises(ValueError, "draw_ids must be int64", sample_items, P, Q, b, users, K, sptr, draw_ids=ids.int())
    raises(ValueError, "users must be int32 or int64", sample_items, P, Q, b, users.float(), K, draw_ids=ids.int())
    raises(ValueError, "draw_ids must have one entry per row of users", sample_items, P, Q, b,
           torch.tensor([U, 1, 2], dtype=torch.int32, device=t["dev"]), K, draw_ids=ids[:2])
    raises(RuntimeError, "sample_items needs every tensor on the device of P", sample_items, P, Q, b, users, K,
           draw_ids=ids.cpu())


def test_neighbors_refuses_behind_the_device_check(t):
    from revisit_bpr.similar import neighbors, similar_items

    P, Q, dev = t["P"], t["Q"], t["dev"]
    rows = torch.tensor([1, 2, 7], dtype=torch.int32, device=dev)
    share = "X [*, d] and T [N, d] must share the embedding dim"
    for message, args, kw in [
        ("T must be float32", (Q.double(), Q.double(), rows, K), {}),
        ("T must be float32", (P.double(), Q.double(), rows, K), {}),  # T is looked at first
        ("X must be float32", (P.double(), Q, rows, K), {}),
        (share, (P[:, :3], Q, rows, K), {}), (share, (P[0], Q, rows, K), {}), (share, (P, Q[0], rows, K), {}),
        ("exclude must have one entry per query", (P, Q, rows, K), dict(exclude=rows[:2])),
        ("row id out of range", (P, Q, torch.tensor([U], device=dev), K), {}),
        ("row id out of range", (P, Q, torch.tensor([-1], device=dev), K), {}),
        ("row id out of range", (Q, Q, torch.tensor([I], device=dev), K), {}),
        ("exclude id out of range", (P, Q, rows, K), dict(exclude=torch.tensor([1, I, 2], device=dev))),
        ("X must be float32", (P.double(), Q[:, :3], rows, K), {}),
        (share, (P[:, :3], Q, rows, K), dict(exclude=rows[:2])),
        ("exclude must have one entry per query", (P, Q, torch.tensor([U, 1, 2], device=dev), K),
         dict(exclude=rows[:2])),
        ("row id out of range", (P, Q, torch.tensor([U, 1, 2], device=dev), K),
         dict(exclude=torch.tensor([1, I, 2], device=dev))),
    ]:
        raises(ValueError, message, neighbors, *args, **kw)
    rocm = "neighbors needs the tables and the row list on a ROCm device; there is no CPU path in libbprcore"
    raises(RuntimeError, rocm, neighbors, P, Q.cpu(), rows, K)
    raises(RuntimeError, rocm, neighbors, P, Q, rows.cpu(), K)
    raises(RuntimeError, rocm, neighbors, P, Q, rows, K, exclude=rows.cpu())
    raises(RuntimeError, rocm, neighbors, P.double(), Q, rows.cpu(), K)
    raises(ValueError, "first must be at least 0", neighbors, P, Q.cpu(), rows, K, first=-1)
    # an entry of `exclude` below 0 excludes nothing and is not refused; any dtype of ids is converted
    want = similar_items(Q, rows, K, "dot")
    for kind in (torch.int64, torch.float64):
        got = similar_items(Q, rows.to(kind).reshape(N, 1), K, "dot")
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    loose = neighbors(Q, Q, rows.long(), K, metric="dot", exclude=torch.full((N,), -1, device=dev), first=1)
    assert loose[0].shape == (N, K) and int(loose[0].min()) >= 1


def test_diversify_refuses_behind_the_device_check(t):
    from revisit_bpr.diversify import diversify, recommend_diverse

    P, Q, b, users, dev = t["P"], t["Q"], t["b"], t["users"], t["dev"]
    ci = torch.tensor([[4, 5, 6], [7, 8, 9], [1, 2, 3]], dtype=torch.int32, device=dev)
    cs = torch.tensor([[3.0, 2.0, 1.0]] * 3, device=dev)
    rocm = "diversify needs the item table and the candidates on a ROCm device; there is no CPU path in libbprcore"
    raises(RuntimeError, rocm, diversify, Q.cpu(), ci, cs, K)
    raises(RuntimeError, rocm, diversify, Q, ci.cpu(), cs, K)
    raises(RuntimeError, rocm, diversify, Q, ci, cs.cpu(), K)
    raises(ValueError, "cand_scores must be float32", diversify, Q, ci.cpu(), cs.double(), K)  # dtypes come first
    raises(ValueError, "Q must be float32", diversify, Q.double(), ci.cpu(), cs, K)
    raises(ValueError, "cand_items and cand_scores must have the same shape", diversify, Q, ci, cs[:2], K)
    raises(ValueError, "user id out of range", recommend_diverse, P, Q, b,
           torch.tensor([U], dtype=torch.int32, device=dev), K, pool=4)
    # lam = 1 is the pool in (score, id) order, whatever dtype the user list of the first stage had
    want = recommend_diverse(P, Q, b, users, K, pool=4, lam=1.0)
    for kind in (torch.int64, torch.float64):
        got = recommend_diverse(P, Q, b, users.to(kind), K, pool=4, lam=1.0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    one = diversify(Q, ci[0], cs[0], K, lam=1.0)
    assert one[0].tolist() == [4, 5] and one[1].tolist() == [3.0, 2.0]
