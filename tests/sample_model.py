"""The sampling kernel's draw, restated exactly on the host: test infrastructure, nothing of it comes from the code
under test.  revisit-bpr_amd/csrc/bpr_sample_shared.h states the contract — the Philox block and word of a (row, item)
pair, the uniform, the logarithm as a fixed sequence of fp32 operations, the Gumbel noise and the key — and this file
is that header in numpy, with the correctly rounded fma of tests/chain_model.py, so that a GPU test can hold
`bpr_sample_rows` to it bit for bit (tests/test_gpu_sample.py) and a CPU test can hold the logarithm to float64 over
every uniform there is and the draws to the Plackett-Luce distribution (tests/test_sample_model_cpu.py)."""
import numpy as np

from chain_model import F, chain_scores, fma32, select

U32, U64, I32 = np.uint32, np.uint64, np.int32
PURPOSE_GUMBEL = 3  # bpr_device.h has 0 and 1 (the two samplers), bpr_foldin_items_roles.hip has 2 (PURPOSE_ROLE)
UNIFORM_BITS = 23   # a uniform is ((bits >> 9) + 0.5f) * 2^-23: every value exact in fp32, strictly inside (0, 1)

# ---- Philox4x32-10 (bpr_device.h), vectorised -------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = U64(0xD2511F53), U64(0xCD9E8D57), U64(0x9E3779B9), U64(0xBB67AE85)
_LO = U64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the four output words (uint32 arrays) of the block with counter (c0, c1, c2, c3) under key (k0, k1)"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v).astype(U64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> U64(32)) ^ c1 ^ k0) & _LO, p1 & _LO, ((p0 >> U64(32)) ^ c3 ^ k1) & _LO, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0.astype(U32), c1.astype(U32), c2.astype(U32), c3.astype(U32)


def gumbel_bits(draw_ids, items, seed):
    """the 32 random bits of every (row, item) pair, uint32 [n, m]: word `i & 3` of the block whose counter is
    (i >> 2, lo(draw_id), hi(draw_id), PURPOSE_GUMBEL) under the key (lo(seed), hi(seed))"""
    did = np.asarray(draw_ids).astype(np.int64).view(U64).reshape(-1, 1)
    it = np.asarray(items).astype(U64).reshape(1, -1)
    seed = U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    w = philox4x32_10(it >> U64(2), did & _LO, did >> U64(32), U64(PURPOSE_GUMBEL), seed & _LO, seed >> U64(32))
    word = np.broadcast_to(it & U64(3), w[0].shape)
    return np.choose(word.astype(np.int64), w)


# ---- the uniform, the logarithm, the noise ----------------------------------------------------------------------------
def uniform(bits):
    """u = ((bits >> 9) + 0.5f) * 2^-23: both operations are exact (2 n + 1 < 2^24), u is strictly inside (0, 1)"""
    n = (np.asarray(bits, U32) >> U32(32 - UNIFORM_BITS)).astype(F)
    return ((n + F(0.5)).astype(F) * F(2.0 ** -UNIFORM_BITS)).astype(F)


_SQRT_HALF = 0x3F3504F3  # bits of fl32(sqrt(1/2))
LOG_POLY = (7.0376836292e-2, -1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1,
            -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1)
LN2_HI, LN2_LO = 0.693359375, -2.12194440e-4


def log32(x):
    """bpr_sample_shared.h, sample_log: the natural logarithm of a positive, normal, finite float32 as a fixed
    sequence of fp32 operations.  x = m * 2^e with m in [sqrt(1/2), sqrt(2)) by integer operations on the bits;
    f = m - 1 (exact); p = Horner over LOG_POLY in f, one fma a step; z = f * f; t = f * z; y = t * p;
    y = fma(e, LN2_LO, y); y = fma(-0.5, z, y); r = f + y; r = fma(e, LN2_HI, r)."""
    x = np.asarray(x, F)
    ix = (x.view(U32).astype(np.int64) - _SQRT_HALF)
    e = (ix >> 23).astype(F)  # (ix >= 0 for every x >= sqrt(1/2); below, the arithmetic shift of the device)
    m = ((ix & 0x007FFFFF) + _SQRT_HALF).astype(U32).view(F)
    f = (m - F(1)).astype(F)
    p = np.full(x.shape, F(LOG_POLY[0]), F)
    for c in LOG_POLY[1:]:
        p = fma32(p, f, F(c))
    z = (f * f).astype(F)
    t = (f * z).astype(F)
    y = (t * p).astype(F)
    y = fma32(e, F(LN2_LO), y)
    y = fma32(F(-0.5), z, y)
    r = (f + y).astype(F)
    return fma32(e, F(LN2_HI), r)


def gumbel(u):
    """g = -log(-log(u)), with log32 both times; the negations are exact"""
    return (-log32((-log32(u)).astype(F))).astype(F)


def keys(scores, inv_temp, draw_ids, items, seed):
    """key[r, i] = fma(score[r, i], inv_temp, g[r, i]) for scores [n, m] of the items `items` [m]"""
    g = gumbel(uniform(gumbel_bits(draw_ids, items, seed)))
    return fma32(np.asarray(scores, F), F(inv_temp), g)


def inv_temperature(temperature):
    """1.0f / temperature in fp32, as the host computes it"""
    return F(1) / F(temperature)


# ---- the call ---------------------------------------------------------------------------------------------------------
def eligible(n_items, users, indptr, indices):
    """[n, I] bool: item 0 and the user's seen row are out"""
    ok = np.ones((len(users), n_items), bool)
    ok[:, 0] = False
    if indptr is not None:
        for r, u in enumerate(users):
            ok[r, indices[indptr[u]:indptr[u + 1]]] = False
    return ok


def sample_rows(P, Q, bias, users, k, indptr=None, indices=None, temperature=1.0, seed=0, draw_ids=None):
    """what bpr_sample_rows returns: (items [n, k] int32, scores [n, k], keys [n, k]) and the score matrix used"""
    users = np.asarray(users)
    draw_ids = users if draw_ids is None else draw_ids
    S = chain_scores(P[users], Q, bias)
    K = keys(S, inv_temperature(temperature), draw_ids, np.arange(Q.shape[0]), seed)
    ok = eligible(Q.shape[0], users, indptr, indices)
    cols = np.arange(Q.shape[0])
    items, kk = np.full((len(users), k), -1, I32), np.full((len(users), k), -np.inf, F)
    sc = np.full((len(users), k), -np.inf, F)
    for r in range(len(users)):
        items[r], kk[r] = select(K[r, ok[r]], cols[ok[r]], k)
        have = items[r] >= 0
        sc[r, have] = S[r, items[r, have]]
    return items, sc, kk, S


def log_z64(S, ok, inv_temp):
    """log sum exp(score * inv_temp) over the eligible items whose score is not NaN, in float64 (the product is the
    fp32 one); -inf for a row with nothing eligible, +inf with an eligible +inf"""
    with np.errstate(all="ignore"):
        x = (np.asarray(S, F) * F(inv_temp)).astype(F).astype(np.float64)
        x = np.where(ok & ~np.isnan(x), x, -np.inf)
        m = x.max(axis=1)
        safe = np.where(np.isfinite(m), m, 0.0)
        return np.where(np.isfinite(m), safe + np.log(np.exp(x - safe[:, None]).sum(axis=1)), m)
