"""A numpy model of dynamic negative sampling as DESIGN.md and include/bprcore.h state it (bpr_sample_dynamic,
BPR_NEG_DYNAMIC): the candidate stream from `oracle.philox4x32_10`, acceptance, the pick, the margin inside which the
fp32 kernels may disagree with it, and a sequential trainer.  Shared by tests/test_dynamic_model_cpu.py and
tests/test_gpu_dynamic.py; nothing here needs a GPU.

For triple counter t, seed s, user u and M in 1..32:
  candidate k  = uniform_candidate(philox(s, t, block k >> 2, purpose 0)[k & 3], I, weights), k = 0 .. 4,095
  accepted     = not in seen(u); a_1 .. a_m = the first min(M, accepted) accepted ones in order of k, duplicates kept
  none         = the uniform sampler's exact pick by rank (Philox block 1,024, word 0; item 0 when nothing is unseen)
  score(a)     = <P[u], Q[a]> (+ bias[a]), here in float64
  pick         = a_1, replaced by a_i (i = 2 .. m) when score(a_i) > score(best), or score(best) is NaN and
                 score(a_i) is not

The margin.  A float32 dot product over d terms, summed in any order, is within d * 2^-24 * sum|p_f q_f| of the exact
value (+ one rounding for the bias term), so two float32 scores can order differently from the exact ones only when
the exact ones are closer than 2 * (d + 1) * 2^-24 * max_a (sum|p_f q_af| + |b_a|).  A triple is DECIDED when the
best score leads the best score of any OTHER item by more than that, or when all its scores are bit-equal; picks are
compared on decided triples only.
"""
import numpy as np

import oracle

M32 = 0xFFFFFFFF
UNIFORM_MAX_CAND = 4096
PURPOSE_UNIFORM = 0


def block(seed, t, blk):
    """The four 32-bit words of Philox block `blk` of the uniform stream for (seed, counter t)."""
    return oracle.philox4x32_10((t & M32, (t >> 32) & M32, blk, PURPOSE_UNIFORM), (seed & M32, (seed >> 32) & M32))


def uniform_candidate(r, I, accept=None, alias=None):
    """bpr_device.h uniform_candidate: column 1 + floor(r (I-1) / 2^32); with item weights the fractional part decides
    between the column and its alias (fp32 arithmetic, as the kernel's)."""
    n = I - 1
    c = 1 + ((r * n) >> 32)
    if accept is None:
        return c
    frac = np.float32((r * n) & M32) * np.float32(1.0 / 4294967296.0)
    return c if frac < accept[c] else int(alias[c])


def candidates(seed, t, I, accept=None, alias=None):
    """Candidate k = 0 .. 4,095 of triple t, lazily."""
    for blk in range(UNIFORM_MAX_CAND // 4):
        for r in block(seed, t, blk):
            yield uniform_candidate(r, I, accept, alias)


def accepted(seed, t, seen, I, M, accept=None, alias=None):
    """a_1 .. a_m: the first min(M, accepted) candidates not in `seen` (a set), in order of k."""
    out = []
    for c in candidates(seed, t, I, accept, alias):
        if c not in seen:
            out.append(c)
            if len(out) == M:
                break
    return out


def rank_pick(seed, t, seen, I):
    """The uniform sampler's exact fallback: item number mulhi32(word 0 of block 1,024, #unseen) among the unseen
    items 1 .. I-1 in ascending order; 0 when nothing is unseen."""
    unseen = [i for i in range(1, I) if i not in seen]
    if not unseen:
        return 0
    r = block(seed, t, UNIFORM_MAX_CAND // 4)[0]
    return unseen[(r * len(unseen)) >> 32]


def scores(p, Q, bias, items):
    """(score, sum|p q| + |b|) per item, float64."""
    rows = Q[items].astype(np.float64)
    p = p.astype(np.float64)
    prod = rows * p
    b = np.zeros(len(items)) if bias is None else bias[items].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return prod.sum(1) + b, np.abs(prod).sum(1) + np.abs(b)


def choose(s):
    """Index of the pick among scores s (the rule above)."""
    best = 0
    for i in range(1, len(s)):
        if s[i] > s[best] or (np.isnan(s[best]) and not np.isnan(s[i])):
            best = i
    return best


def margin(d, mags):
    finite = mags[np.isfinite(mags)]
    return 2.0 * (d + 1) * 2.0 ** -24 * (float(finite.max()) if finite.size else 0.0)


def pick(seed, t, u, M, P, Q, bias, indptr, indices, accept=None, alias=None, seen=None, pre=None):
    """The model's draw for one triple.  Returns a dict: item, score (float64), cands (a_1 .. a_m, or the rank pick
    alone), accepted (how many of the 4,096 candidates made the list: 0 = rank pick), decided, margin.
    pre: the triple's accepted list for some M' >= M (`accepted_lists`): a_1 .. a_m is its prefix."""
    I, d = Q.shape
    if seen is None:
        seen = set(indices[indptr[u]:indptr[u + 1]].tolist())
    a = list(pre[:M]) if pre is not None else accepted(seed, t, seen, I, M, accept, alias)
    n_acc = len(a)
    if not a:
        a = [rank_pick(seed, t, seen, I)]
    items = np.asarray(a, np.int64)
    s, mags = scores(P[u], Q, bias, items)
    k = choose(s)
    mg = margin(d, mags)
    others = s[(items != items[k]) & ~np.isnan(s)]
    bit_equal = bool(np.all(s.view(np.uint64) == s.view(np.uint64)[0]))
    if np.isnan(s[k]):  # every score is NaN: a_1, whatever the arithmetic
        decided = True
    else:
        decided = bit_equal or others.size == 0 or bool(s[k] - others.max() > mg)
    return dict(item=int(items[k]), score=float(s[k]), cands=a, accepted=n_acc, decided=decided, margin=mg)


def accepted_lists(indptr, indices, I, users, M, seed, offset=0, accept=None, alias=None):
    """Per entry of `users` its accepted list a_1 .. a_m for M candidates: they depend on neither the tables nor the
    width, so the tests that sweep those compute them once (for the largest M) and share them."""
    seen_of, out = {}, []
    for b, u in enumerate(users.tolist()):
        if u not in seen_of:
            seen_of[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
        out.append(accepted(seed, offset + b, seen_of[u], I, M, accept, alias))
    return out


def sample(P, Q, bias, indptr, indices, users, M, seed, offset=0, accept=None, alias=None, lists=None):
    """The model of bpr_sample_dynamic on static tables: (items int32 [B], scores float64 [B], decided bool [B],
    margins float64 [B], accepted int [B]).  lists: `accepted_lists` of the same draws for an M' >= M."""
    B = len(users)
    items, sc = np.zeros(B, np.int32), np.zeros(B)
    dec, mg, acc = np.zeros(B, bool), np.zeros(B), np.zeros(B, np.int64)
    seen_of = {}
    for b, u in enumerate(users.tolist()):
        if u not in seen_of:
            seen_of[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
        r = pick(seed, offset + b, u, M, P, Q, bias, indptr, indices, accept, alias, seen_of[u],
                 None if lists is None else lists[b])
        items[b], sc[b], dec[b], mg[b], acc[b] = r["item"], r["score"], r["decided"], r["margin"], r["accepted"]
    return items, sc, dec, mg, acc


def train_sequential(P, Q, bias, indptr, indices, users, pos, M, lr, alphas, seed, offset=0):
    """One triple at a time: the pick from the live rows, then oracle.step_sgd_sparse with B = 1.  P, Q, bias are
    updated in place.  Returns (negatives int32 [n], decided bool [n], scalars float64 [4])."""
    n = len(users)
    neg, dec = np.zeros(n, np.int32), np.zeros(n, bool)
    sc = np.zeros(4)
    seen_of = {}
    for t in range(n):
        u = int(users[t])
        if u not in seen_of:
            seen_of[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
        r = pick(seed, offset + t, u, M, P, Q, bias, indptr, indices, seen=seen_of[u])
        neg[t], dec[t] = r["item"], r["decided"]
        _, _, s = oracle.step_sgd_sparse(P, Q, bias, users[t:t + 1], pos[t:t + 1], neg[t:t + 1], lr, alphas)
        sc += s
    return neg, dec, sc


def rank_pmf(N, M):
    """P(rank of the pick = r), r = 1 .. N (1 = best), for M candidates drawn uniformly with replacement from N items
    with distinct scores: the maximum of M draws."""
    r = np.arange(1, N + 1, dtype=np.float64)
    return ((N - r + 1) ** M - (N - r) ** M) / float(N) ** M


def chi2_sf(x, dof):
    """Survival function of the chi-square distribution, Q(dof / 2, x / 2): the regularized upper incomplete gamma
    function by its series (x < a + 1) or continued fraction (Numerical Recipes 6.2), in plain Python."""
    import math

    a, x = dof / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        ap = a
        for _ in range(10000):
            ap += 1.0
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    dd = 1.0 / b
    h = dd
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        dd = an * dd + b
        dd = tiny if abs(dd) < tiny else dd
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        dd = 1.0 / dd
        delta = dd * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return math.exp(-x + a * math.log(x) - lg) * h
