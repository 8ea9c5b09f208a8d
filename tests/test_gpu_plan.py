"""The epoch planner and the shuffle — bpr_plan_epoch, bpr_plan_chunk (bpr_plan.hip) and bpr_shuffle_epoch
(k_shuffle_scatter) — against their numpy restatement (tests/plan_model.py, itself held to published vectors and to
the algebra of a permutation in tests/test_plan_model_cpu.py).  All of it is integer work: every comparison here is
`np.array_equal`, there is no tolerance anywhere.

Each case that names a route of the host code (32- or 64-bit sort keys, the bucket kernels' layout, the device-wide
sort) asserts that route through the model's `key_bits` / `chunk_route`, so that it cannot silently move to another.
The tables are d = 4 (the planner never reads them), so U = 2^21 + 1 rows are 32 MB."""
import numpy as np
import pytest

import plan_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

I = 300
SEEDS = [1, 5 + 2**32, 2**64 - 1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_engine(U, d=4):
    from revisit_bpr.engine import Engine

    Q = np.random.default_rng(0).normal(0, 0.1, (I, d)).astype(np.float32)  # (the split refresh sorts its columns)
    return Engine(torch.zeros((U, d), dtype=torch.float32, device="cuda"), dev(Q))


def draw(rng, n, U, lo=0, hi=None):
    """n (user, positive) pairs, the two columns independent; ids 0 and U - 1 are always among the users."""
    users = rng.integers(lo, U if hi is None else hi, n).astype(np.int32)
    edge = rng.permutation(n)[:2]
    users[edge] = np.array([U - 1, 0], np.int32)[:len(edge)]
    return users, rng.integers(1, I, n).astype(np.int32)


def empty_pair(m, fill=None):
    if fill is None:
        return tuple(torch.empty(m, dtype=torch.int32, device="cuda") for _ in range(2))
    return tuple(torch.full((m,), fill, dtype=torch.int32, device="cuda") for _ in range(2))


def host(pair):
    return tuple(t.cpu().numpy() for t in pair)


def assert_plan(e, users, pos, U, chunk, seed, **kw):
    want_u, want_p = pm.plan_epoch(users, pos, U, chunk, seed)
    got_u, got_p = host(e.plan_epoch(dev(users), dev(pos), chunk, seed, **kw))
    assert np.array_equal(got_u, want_u), (users.size, chunk, U, seed, kw)
    assert np.array_equal(got_p, want_p), (users.size, chunk, U, seed, kw)
    return want_u, want_p


def assert_chunk(e, u_d, p_d, users, pos, chunk, seed, index, on_side=False):
    """plan_chunk(index) against the model: the user column identical, the positives identical per user."""
    m = min(chunk, users.size - index * chunk)
    out = empty_pair(m, fill=-7)
    if on_side:
        e.adaptive_refresh_begin()
    e.plan_chunk(u_d, p_d, chunk, seed, index, out, on_side=on_side)
    if on_side:
        e.adaptive_refresh_commit()  # the launch stream now waits for the sort and the plan
    got_u, got_p = host(out)
    want_u, want_p = pm.plan_chunk_members(users, pos, chunk, seed, index)
    assert want_u.size == m
    assert np.array_equal(got_u, want_u), (users.size, chunk, seed, index, on_side)
    assert np.array_equal(pm.canon(got_u, got_p)[1], pm.canon(want_u, want_p)[1]), (users.size, chunk, seed, index)


# ---- 1. plan_epoch, both columns ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk,U", [
    (777, 100, 60), (100_000, 9_984, 5000),                            # the shapes the property tests use
    (5, 2, 3), (17, 4, 9), (4_097, 1_000, 700), (65_537, 9_984, 5000),  # n = 4^k + 1: tens of cycle-walk passes
    (1, 1, 2), (1, 7, 5),                                              # one triple
    (777, 777, 60), (777, 1_000, 60),                                  # one chunk: chunk = n, chunk > n
    (777, 1, 60),                                                      # every triple a chunk of its own
])
def test_plan_epoch_equals_the_model(n, chunk, U):
    rng = np.random.default_rng(n * 31 + chunk)
    users, pos = draw(rng, n, U)
    assert sum(pm.key_bits(U, n, chunk)) < 32
    e = make_engine(U)
    for seed in SEEDS:
        assert_plan(e, users, pos, U, chunk, seed)


# ---- 2. the key-width routes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,n,chunk,bits", [
    (2**20, 8192, 2, 32),      # 20 + 12: the 32-bit route with end_bit = 32, the chunk index fills the top bit
    (2**20 + 1, 8192, 2, 33),  # 21 + 12: 64-bit keys
    (2**20 + 1, 8193, 2, 34),  # 21 + 13
])
def test_plan_epoch_key_width_routes(U, n, chunk, bits):
    """Unsorted users against the model; then users sorted by id, where `sorted_input=True` (the radix sort starts at
    begin_bit = ubits) must give the plan `sorted_input=False` gives, and both the model's.  A quarter of the users is
    U - 1 and the triples of the highest chunks carry it, so the top bits of user and chunk are live together.

    The 32-bit case with `sorted_input=True` is the regression test of a wrong plan: sorting 8,192 32-bit keys on the
    bits [20, 32) merges them under a mask built with a shift by the key's whole width, which left the user bits in it
    — the plan came out ordered by user across the chunks.  plan_epoch_impl sorts that one case on 64-bit keys now."""
    ubits, cbits = pm.key_bits(U, n, chunk)
    assert ubits + cbits == bits and (bits > 32) == (U > 2**20)
    n_chunks = -(-n // chunk)
    rng = np.random.default_rng(bits)
    users, pos = draw(rng, n, U)
    users[rng.random(n) < 0.25] = U - 1
    e = make_engine(U)
    for seed in SEEDS:
        p, _ = pm.perm(n, seed, 4)
        top = users.copy()
        top[p // chunk >= n_chunks - 4] = U - 1
        want_u, _ = assert_plan(e, top, pos, U, chunk, seed)
        assert want_u[-1] == U - 1
        order = np.argsort(users, kind="stable")
        su, sp = users[order], pos[order]
        want_u, _ = assert_plan(e, su, sp, U, chunk, seed)
        assert (want_u[-64:] == U - 1).any()  # the largest user id in the highest chunks
        assert_plan(e, su, sp, U, chunk, seed, sorted_input=True)
        a = e.plan_epoch(dev(su), dev(sp), chunk, seed, sorted_input=True)
        b = e.plan_epoch(dev(su), dev(sp), chunk, seed, sorted_input=False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 3. plan_chunk, every index of the plan ------------------------------------------------------------------------------
def _users_all(rng, n, U):
    return draw(rng, n, U)


def _users_top_bucket(rng, n, U):  # half of the triples in the last 1,024 ids: one workgroup's counting sort is full
    users, pos = draw(rng, n, U)
    crowd = rng.random(n) < 0.5
    users[crowd] = rng.integers(U - 1024, U, int(crowd.sum())).astype(np.int32)
    return users, pos


def _users_edges(rng, n, U):  # ids 0 and U - 1 only
    users, pos = draw(rng, n, U)
    return np.where(rng.random(n) < 0.5, 0, U - 1).astype(np.int32), pos


def _users_one(rng, n, U):  # one user owns every chunk: sz = m in one workgroup of k_pc_group
    users, pos = draw(rng, n, U)
    return np.full(n, U * 2 // 3, np.int32), pos


@pytest.mark.parametrize("U,n,chunk,route,users_of", [
    (2, 1_000, 300, ("buckets", 0, 2), _users_all),
    (2048, 20_000, 4_096, ("buckets", 0, 2048), _users_all),           # L = 1, the most buckets
    (2049, 20_000, 4_096, ("buckets", 1, 1025), _users_all),           # the last bucket holds one id
    (2**21, 50_000, 9_984, ("buckets", 10, 2048), _users_top_bucket),  # L = 1024, nb = 2048: the largest layout
    (2**21, 3_000, 1_024, ("buckets", 10, 2048), _users_edges),
    (2**21 + 1, 50_000, 9_984, ("sort",), _users_top_bucket),          # the device-wide sort, no environment variable
    (5000, 3_000, 1_024, ("buckets", 2, 1250), _users_one),
    (5000, 3_000, 1_024, ("buckets", 2, 1250), _users_edges),
    (60, 777, 100, ("buckets", 0, 60), _users_all),                    # m below one workgroup
    (60, 7, 1, ("buckets", 0, 60), _users_all),                        # m = 1
])
def test_plan_chunk_equals_the_model_at_every_index(U, n, chunk, route, users_of):
    assert pm.chunk_route(U) == route
    rng = np.random.default_rng(U + n)
    users, pos = users_of(rng, n, U)
    e = make_engine(U)
    u_d, p_d = dev(users), dev(pos)
    for seed in SEEDS[:2] if n > 10_000 else SEEDS:
        for index in range(-(-n // chunk)):
            assert_chunk(e, u_d, p_d, users, pos, chunk, seed, index)
        # and the epoch plan of the same engine is the concatenation of these chunks
        assert_plan(e, users, pos, U, chunk, seed)


@pytest.mark.parametrize("first_on_side", [False, True])
def test_plan_chunk_counters_survive_chunks_of_changing_size(first_on_side):
    """One engine, chunks of 100, then 9,984 (the scratch buffers and the counters are reallocated), then the short last
    chunk, 1 and 100 again: the bucket counters zero themselves for the next chunk whatever its size.  With
    `first_on_side` the first call — the one that allocates and zeroes the counters — runs on the split refresh's side
    stream, and the launch stream's calls that follow are ordered behind it only through the commit."""
    U, n = 5000, 30_000
    assert pm.chunk_route(U) == ("buckets", 2, 1250)
    rng = np.random.default_rng(9)
    users, pos = draw(rng, n, U)
    e = make_engine(U, d=32)
    e.adaptive_refresh()
    u_d, p_d = dev(users), dev(pos)
    seed = SEEDS[1]
    steps = [(100, 3), (100, 299), (9_984, 0), (9_984, 3), (100, 7), (1, 12_345), (1, n - 1), (9_984, 2), (100, 0),
             (20_000, 1), (20_000, 0), (1, 0)]
    for k, (chunk, index) in enumerate(steps):
        assert_chunk(e, u_d, p_d, users, pos, chunk, seed, index, on_side=first_on_side and k == 0)


def test_plan_chunk_on_the_side_stream():
    """Every other chunk queued on the side stream behind a split refresh in flight."""
    U, n, chunk = 2049, 20_000, 4_096
    rng = np.random.default_rng(4)
    users, pos = draw(rng, n, U)
    e = make_engine(U, d=32)
    e.adaptive_refresh()
    u_d, p_d = dev(users), dev(pos)
    for index in range(-(-n // chunk)):
        assert_chunk(e, u_d, p_d, users, pos, chunk, 7, index, on_side=index % 2 == 0)


def test_plan_chunk_past_the_end_writes_nothing():
    U, n, chunk = 60, 777, 100
    rng = np.random.default_rng(5)
    users, pos = draw(rng, n, U)
    e = make_engine(U)
    u_d, p_d = dev(users), dev(pos)
    out = empty_pair(chunk, fill=-7)
    for index in (8, 9, 2**40):  # n_chunks = 8: at the end, past it, far past it
        e.plan_chunk(u_d, p_d, chunk, 1, index, out)  # OK: nothing to plan
    e.plan_chunk(u_d, p_d, n, 1, 1, out)  # (one chunk of n: index 1 is the end)
    assert all((t == -7).all().item() for t in out)
    assert_chunk(e, u_d, p_d, users, pos, chunk, 1, 7)  # the short last chunk: 77 triples


# ---- 4. shuffle_epoch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 1000, 4_097, 65_536, 65_537, 96_126])
def test_shuffle_epoch_equals_the_model(n):
    rng = np.random.default_rng(n)
    users, pos = draw(rng, n, 5000)  # two independent columns: neither is a function of the other
    e = make_engine(5000)
    u_d, p_d = dev(users), dev(pos)
    for seed in SEEDS:
        want_u, want_p = pm.shuffle_epoch(users, pos, seed)
        got_u, got_p = host(e.shuffle_epoch(u_d, p_d, seed))
        assert np.array_equal(got_u, want_u), (n, seed)
        assert np.array_equal(got_p, want_p), (n, seed)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    from revisit_bpr import native

    U, n, chunk = 60, 777, 100
    rng = np.random.default_rng(6)
    users, pos = draw(rng, n, U)
    e = make_engine(U, d=32)
    u_d, p_d = dev(users), dev(pos)
    out = empty_pair(chunk, fill=-7)
    none = empty_pair(0)
    with pytest.raises(native.BprError):  # n = 0
        e.plan_chunk(none[0], none[1], chunk, 1, 0, out)
    with pytest.raises(native.BprError):  # chunk = 0
        e.plan_chunk(u_d, p_d, 0, 1, 0, out)
    with pytest.raises(native.BprError):  # a negative index
        e.plan_chunk(u_d, p_d, chunk, 1, -1, out)
    with pytest.raises(native.BprError):  # on_side, no split refresh in flight: not even a side stream yet
        e.plan_chunk(u_d, p_d, chunk, 1, 0, out, on_side=True)
    e.adaptive_refresh()
    e.adaptive_refresh_begin()
    e.adaptive_refresh_commit()
    with pytest.raises(native.BprError):  # ... and with a side stream, but the refresh committed
        e.plan_chunk(u_d, p_d, chunk, 1, 0, out, on_side=True)
    other = empty_pair(n)
    with pytest.raises(native.BprError):  # an output aliasing an input, either column
        e.shuffle_epoch(u_d, p_d, 1, out=(u_d, other[1]))
    with pytest.raises(native.BprError):
        e.shuffle_epoch(u_d, p_d, 1, out=(other[0], p_d))
    assert all((t == -7).all().item() for t in out)
    assert np.array_equal(u_d.cpu().numpy(), users) and np.array_equal(p_d.cpu().numpy(), pos)
    assert_plan(e, users, pos, U, chunk, 7)
    assert_chunk(e, u_d, p_d, users, pos, chunk, 7, 3)
