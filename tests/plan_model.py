"""The epoch planner and the shuffle, restated in numpy from the contract in include/bprcore.h (bpr_plan_epoch,
bpr_plan_chunk, bpr_shuffle_epoch) and the comments of the kernels: no GPU work, uint64 arithmetic throughout.

The permutation.  A balanced Feistel network on [0, 4^half_bits) — two halves of half_bits bits, the round function
`mix32(r ^ round_key) & mask` (mix32: the murmur3 finaliser) — is a bijection of that domain whatever the round function
is; re-applying it to an image that fell at or past n until it lands below n ("cycle-walking") makes it a bijection of
[0, n).  Four rounds plan the STREAM epoch, six shuffle the batched one.

The plan.  Triple t goes to chunk perm4(t) // chunk; one STABLE sort by (chunk, user) makes every chunk contiguous and
grouped by user, and leaves the triples of one (chunk, user) group in input order: the whole plan is deterministic.
`plan_chunk_members` finds one chunk through the inverse permutation; there the order inside one user is unspecified.

`key_bits` and `chunk_route` restate which route the host code takes for a shape (32- or 64-bit sort keys; the three
bucket kernels or the device-wide sort), so that a test can assert it sits on the route it claims to cover."""
import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
GOLDEN = 0x9E3779B9
PC_MAX_BUCKETS, PC_MAX_LOCAL = 2048, 1024  # plan_chunk's bucket layout: <= 2048 buckets of <= 1024 consecutive ids


def mix32(x):
    """murmur3's fmix32 on uint64 arrays (or ints) holding 32-bit values."""
    x = np.asarray(x, U64) & M32
    x = x ^ (x >> U64(16))
    x = (x * U64(0x85EBCA6B)) & M32
    x = x ^ (x >> U64(13))
    x = (x * U64(0xC2B2AE35)) & M32
    x = x ^ (x >> U64(16))
    return x


def bits_for(v: int) -> int:
    """Bits needed to represent the values 0..v (one bit for v = 0)."""
    return max(1, int(v).bit_length())


def half_bits(n: int) -> int:
    return max(1, (bits_for(n - 1) + 1) // 2)


def round_key(seed: int, r: int) -> int:
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (((seed >> (16 * (r & 1))) & 0xFFFFFFFF) + GOLDEN * (r + 1) + (seed >> 32)) & 0xFFFFFFFF


def _network(x, hb: int, seed: int, rounds: int, inverse: bool):
    mask = U64((1 << hb) - 1)
    left, right = (x >> U64(hb)) & mask, x & mask
    if not inverse:
        for r in range(rounds):
            left, right = right, left ^ (mix32(right ^ U64(round_key(seed, r))) & mask)
    else:
        for r in reversed(range(rounds)):
            left, right = right ^ (mix32(left ^ U64(round_key(seed, r))) & mask), left
    return (left << U64(hb)) | right


def _walk(x, n: int, seed: int, rounds: int, inverse: bool):
    """The network on every element, then again on those still >= n; -> (images, passes)."""
    hb = half_bits(n)
    x = np.array(x, U64, copy=True).reshape(-1)
    todo = np.arange(x.size)
    passes = 0
    while todo.size:
        x[todo] = _network(x[todo], hb, seed, rounds, inverse)
        todo = todo[x[todo] >= U64(n)]
        passes += 1
    return x.astype(np.int64), passes


def perm(n: int, seed: int, rounds: int, x=None):
    """pi(x) for x in `x` (default: all of [0, n)), and the number of walk passes the slowest element took."""
    return _walk(np.arange(n) if x is None else x, n, seed, rounds, False)


def perm_inv(n: int, seed: int, rounds: int, y=None):
    return _walk(np.arange(n) if y is None else y, n, seed, rounds, True)


def key_bits(U: int, n: int, chunk: int):
    """(ubits, cbits) of the planner's sort key `chunk_index << ubits | user`: 32-bit keys iff the sum is <= 32."""
    n_chunks = -(-n // chunk)
    return bits_for(U - 1), bits_for(n_chunks - 1)


def chunk_route(U: int):
    """("buckets", shift, nb): the three bucket kernels with nb buckets of 2^shift ids; ("sort",): device-wide sort."""
    shift = max(0, bits_for(U - 1) - 11)
    if (1 << shift) <= PC_MAX_LOCAL:
        return ("buckets", shift, ((U - 1) >> shift) + 1)
    return ("sort",)


def plan_epoch(users, pos, U: int, chunk: int, seed: int):
    users, pos = np.asarray(users), np.asarray(pos)
    n = users.size
    if n == 0:
        return users.copy(), pos.copy()
    ubits, _ = key_bits(U, n, chunk)
    p, _ = perm(n, seed, 4)
    key = ((p // chunk).astype(U64) << U64(ubits)) | users.astype(np.int64).astype(U64)
    order = np.argsort(key, kind="stable")
    return users[order], pos[order]


def plan_chunk_members(users, pos, chunk: int, seed: int, index: int):
    """Chunk `index` of the plan, grouped by user (a stable sort here; the order inside one user is unspecified)."""
    users, pos = np.asarray(users), np.asarray(pos)
    n = users.size
    j0 = index * chunk
    t, _ = perm_inv(n, seed, 4, np.arange(j0, min(j0 + chunk, n)))
    order = np.argsort(users[t], kind="stable")
    return users[t][order], pos[t][order]


def shuffle_epoch(users, pos, seed: int):
    users, pos = np.asarray(users), np.asarray(pos)
    uo, po = np.empty_like(users), np.empty_like(pos)
    if users.size:
        p, _ = perm(users.size, seed, 6)
        uo[p], po[p] = users, pos
    return uo, po


def canon(users, pos):
    """Sort the positives inside each user of a by-user-sorted chunk (plan_chunk leaves that order unspecified)."""
    users, pos = np.asarray(users), np.asarray(pos)
    order = np.lexsort((pos, users))
    return users[order], pos[order]
