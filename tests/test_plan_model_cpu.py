"""The yardstick of tests/test_gpu_plan.py, on a machine without a GPU: the numpy restatement of the epoch planner and
the shuffle (tests/plan_model.py) held to things that are not the model — published vectors, the algebra of a bijection
and its inverse, the avalanche of the seed, a distributional statement about chunk membership, and the properties
bpr_plan_epoch promises in include/bprcore.h."""
import numpy as np
import pytest

import plan_model as pm

SEEDS = [0, 1, 7, 5 + 2**32, 2**64 - 1]
NS = [1, 2, 3, 4, 5, 16, 17, 777, 4097, 65536, 65537, 100000, 1000003]


def test_known_vectors():
    assert int(pm.mix32(0)) == 0
    assert int(pm.mix32(1)) == 0x514E28B7  # murmur3 fmix32(1), the published vector
    assert [pm.bits_for(v) for v in (0, 4095, 4096, 2**20, 2**21)] == [1, 12, 13, 21, 22]
    assert [pm.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 4096, 4097)] == [1, 1, 1, 2, 2, 3, 6, 7]
    # round_key by hand: seed = 0x0123456789ABCDEF; r = 0 reads bits 0..31, r = 1 bits 16..47, both add the high word
    seed = 0x0123456789ABCDEF
    assert pm.round_key(seed, 0) == (0x89ABCDEF + 0x9E3779B9 + 0x01234567) % 2**32
    assert pm.round_key(seed, 1) == (0x456789AB + 2 * 0x9E3779B9 + 0x01234567) % 2**32
    assert pm.round_key(seed, 4) == (0x89ABCDEF + 5 * 0x9E3779B9 + 0x01234567) % 2**32


def test_routes_of_the_named_shapes():
    """key_bits / chunk_route at the shapes tests/test_gpu_plan.py names, worked out by hand from bits_for."""
    assert pm.key_bits(2**20, 8192, 2) == (20, 12)
    assert pm.key_bits(2**20 + 1, 8192, 2) == (21, 12)
    assert pm.key_bits(2**20 + 1, 8193, 2) == (21, 13)
    assert pm.key_bits(60, 777, 100) == (6, 3)
    assert pm.key_bits(5, 1, 7) == (3, 1)
    assert pm.chunk_route(2) == ("buckets", 0, 2)
    assert pm.chunk_route(2048) == ("buckets", 0, 2048)
    assert pm.chunk_route(2049) == ("buckets", 1, 1025)  # the last bucket holds id 2048 alone
    assert pm.chunk_route(2**21) == ("buckets", 10, 2048)
    assert pm.chunk_route(2**21 + 1) == ("sort",)


@pytest.mark.parametrize("rounds", [4, 6])
@pytest.mark.parametrize("n", NS)
def test_perm_is_a_bijection_and_perm_inv_its_inverse(n, rounds):
    ident = np.arange(n)
    for seed in SEEDS:
        p, _ = pm.perm(n, seed, rounds)
        assert p.min() >= 0 and p.max() < n
        assert np.array_equal(np.sort(p), ident)
        q, _ = pm.perm_inv(n, seed, rounds, p)
        assert np.array_equal(q, ident)
        q, _ = pm.perm_inv(n, seed, rounds)
        assert np.array_equal(np.sort(q), ident)
        back, _ = pm.perm(n, seed, rounds, q)
        assert np.array_equal(back, ident)


@pytest.mark.parametrize("rounds", [4, 6])
def test_walk_depth(rounds):
    """A power of four is the network's whole domain: one pass.  At n = 4^k + 1 the domain is four times n and the last
    element lands only after many passes: with seed 2^64 - 1, 9 passes at n = 5, 26 at n = 4,097 and 47 at n = 65,537
    under 6 rounds, and 5, 33 and 43 under 4 (recorded, not asserted: any count above one shows the walk is
    exercised)."""
    for n in (4, 16, 65536):
        for seed in SEEDS:
            assert pm.perm(n, seed, rounds)[1] == 1 and pm.perm_inv(n, seed, rounds)[1] == 1
    for n in (5, 4097, 65537):
        passes = pm.perm(n, 2**64 - 1, rounds)[1]
        print(f"n = {n}, rounds = {rounds}: {passes} passes")
        assert passes > 1
        assert pm.perm_inv(n, 2**64 - 1, rounds)[1] > 1


@pytest.mark.parametrize("rounds", [4, 6])
@pytest.mark.parametrize("bit", [0, 16, 32, 63])
def test_every_part_of_the_seed_matters(bit, rounds):
    """Seeds that differ in one bit give unrelated permutations: two unrelated permutations agree in about one position
    (Poisson(1)), 1 % of n = 96,126 is 961 of them."""
    n = 96_126
    for base in (0, 5 + 2**32):
        a, _ = pm.perm(n, base, rounds)
        b, _ = pm.perm(n, base ^ (1 << bit), rounds)
        share = float((a == b).mean())
        print(f"bit {bit}, rounds {rounds}, base {base}: agree in {int((a == b).sum())} of {n}")
        assert share < 0.01


@pytest.mark.parametrize("rounds", [4, 6])
def test_chunk_membership_is_uniform_over_the_input(rounds):
    """Which chunk a triple lands in must not depend on where in the input it stands.  For (n, chunk) in {(100000,
    9984), (238753, 24896), (50000, 4096)} and seeds 1..8, tabulate chunk x eighth-of-the-input.  Under a uniformly
    random assignment a cell of a chunk of `size` triples is Binomial(size, 1/8): expectation size / 8, variance
    size / 8 * 7 / 8.  Over the ~2,000 cells the worst |z| of a truly uniform assignment exceeds 5.0 with probability
    about 2,000 * 5.7e-7 ~ 1e-3; the seeds are fixed, so the test is deterministic.  Measured with this model on the
    CPU: worst |z| 3.58 with 4 rounds, 3.35 with 6.  The bound is |z| < 5.0."""
    worst = 0.0
    cells = 0
    for n, chunk in ((100000, 9984), (238753, 24896), (50000, 4096)):
        n_chunks = -(-n // chunk)
        eighth = np.arange(n) * 8 // n
        size = np.minimum(chunk, n - np.arange(n_chunks) * chunk).astype(np.float64)
        for seed in range(1, 9):
            p, _ = pm.perm(n, seed, rounds)
            table = np.zeros((n_chunks, 8))
            np.add.at(table, (p // chunk, eighth), 1)
            assert np.array_equal(table.sum(1), size)
            exp = size[:, None] / 8
            z = np.abs(table - exp) / np.sqrt(exp * 7 / 8)
            worst = max(worst, float(z.max()))
            cells += z.size
    print(f"rounds {rounds}: worst |z| {worst:.2f} over {cells} cells")
    assert worst < 5.0


@pytest.mark.parametrize("n,chunk,U", [(777, 100, 60), (50_000, 4096, 3000), (8193, 2, 2**20 + 1), (5, 7, 3), (1, 1, 2)])
def test_plan_epoch_of_the_model(n, chunk, U):
    rng = np.random.default_rng(n)
    users = rng.integers(0, U, n).astype(np.int32)
    users[:2] = (0, U - 1)[:n]
    pos = rng.integers(1, 300, n).astype(np.int32)
    key = lambda u, p: np.sort(u.astype(np.int64) * 300 + p)
    for seed in (1, 5 + 2**32, 2**64 - 1):
        pu, pp = pm.plan_epoch(users, pos, U, chunk, seed)
        assert np.array_equal(key(pu, pp), key(users, pos))  # a permutation of the input pairs
        for c0 in range(0, n, chunk):
            assert np.all(np.diff(pu[c0:c0 + chunk]) >= 0)  # every chunk sorted by user
        # chunk `index` holds exactly the triples the inverse permutation finds
        n_chunks = -(-n // chunk)
        for index in sorted(set(range(0, n_chunks, max(1, n_chunks // 64))) | {n_chunks - 1}):
            cu, cp = pm.plan_chunk_members(users, pos, chunk, seed, index)
            assert np.array_equal(cu, pu[index * chunk:(index + 1) * chunk])
            assert np.array_equal(pm.canon(cu, cp)[1], pm.canon(cu, pp[index * chunk:(index + 1) * chunk])[1])
        # the plan_input_sorted promise: users sorted by id -> a stable sort on the chunk bits alone is the same plan
        order = np.argsort(users, kind="stable")
        su, sp = users[order], pos[order]
        want_u, want_p = pm.plan_epoch(su, sp, U, chunk, seed)
        by_chunk = np.argsort(pm.perm(n, seed, 4)[0] // chunk, kind="stable")
        assert np.array_equal(su[by_chunk], want_u) and np.array_equal(sp[by_chunk], want_p)


def test_shuffle_epoch_of_the_model():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 1000, 4097):
        users, pos = rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
        su, sp = pm.shuffle_epoch(users, pos, 7)
        p, _ = pm.perm(n, 7, 6)
        assert np.array_equal(su[p], users) and np.array_equal(sp[p], pos)
        q, _ = pm.perm_inv(n, 7, 6)
        assert np.array_equal(su, users[q]) and np.array_equal(sp, pos[q])
