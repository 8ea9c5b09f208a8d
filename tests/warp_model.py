"""A numpy model of the WARP objective as DESIGN.md §4.17 and include/bprcore.h state it (bpr_sample_warp,
BPR_NEG_WARP): the candidate stream from `oracle.philox4x32_10` by way of tests/dynamic_model.py, the first violator,
the rank weight, the comparisons the fp32 kernels may decide differently, and a sequential trainer on
`oracle.step_sgd_sparse`.  Shared by tests/test_warp_model_cpu.py and tests/test_gpu_warp.py; nothing here needs a GPU.

For triple counter t, seed s, user u, positive i, N in 1..32 and margin > 0:
  a_1 .. a_m   = dynamic_model.accepted(s, t, seen(u), I, N) — or the uniform sampler's exact rank pick alone
  x_i, x_k     = <P[u], Q[i]> (+ b_i), <P[u], Q[a_k]> (+ b_{a_k}), here in float64
  violator     = the smallest k with x_k > x_i - margin (NaN compares false); tries = k; none: the triple is skipped
  weight       = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - |seen(u)|

Undecided.  A float32 score is within eps = 2 (d + 1) 2^-24 (sum|p q| + |b|) of the exact one (dynamic_model.py), so
the comparison x_k > x_i - margin is UNDECIDED when |x_k - (x_i - margin)| < eps_k + eps_i.  A triple is undecided if
any comparison up to and including its first SURE violator (decided, and violating) is; exact comparisons leave
undecided triples out.
"""
import math

import numpy as np

import dynamic_model as dm
import oracle

EPS = 2.0 ** -24


def weight(n_unseen, tries):
    return math.log(max(1, n_unseen // tries))


def draw(seed, t, u, i, N, margin, P, Q, bias, indptr, indices, accept=None, alias=None, seen=None, pre=None):
    """The model's draw for one triple.  Returns a dict: item (-1 = skipped), tries (0 = skipped), x_pos, x_neg
    (float64; x_neg 0 when skipped), weight, cands, accepted (0 = the rank pick), undecided, eps (eps_i + the largest
    eps_k looked at).  pre: the triple's accepted list for some N' >= N."""
    I, d = Q.shape
    if seen is None:
        seen = set(indices[indptr[u]:indptr[u + 1]].tolist())
    a = list(pre[:N]) if pre is not None else dm.accepted(seed, t, seen, I, N, accept, alias)
    n_acc = len(a)
    if not a:
        a = [dm.rank_pick(seed, t, seen, I)]
    s, mags = dm.scores(P[u], Q, bias, np.asarray([i] + a, np.int64))
    eps = 2.0 * (d + 1) * EPS * mags
    x_i, e_i = s[0], eps[0]
    out = dict(item=-1, tries=0, x_pos=float(x_i), x_neg=0.0, weight=0.0, cands=a, accepted=n_acc, undecided=False,
               eps=float(e_i))
    first = 0  # the model's violator (float64), 1-based
    for k in range(1, len(a) + 1):
        x_k, e_k = s[k], eps[k]
        if np.isnan(x_k) or np.isnan(x_i):
            continue  # compares false in any arithmetic
        gap = x_k - (x_i - margin)
        und = abs(gap) < e_k + e_i or not np.isfinite(e_k + e_i)
        out["eps"] = max(out["eps"], float(e_i + e_k))
        if und:
            out["undecided"] = True
        if gap > 0 and first == 0:
            first = k
        if gap > 0 and not und:  # the first sure violator: nothing past it is looked at
            break
    if first:
        n_unseen = (I - 1) - len(seen)
        out.update(item=int(a[first - 1]), tries=first, x_neg=float(s[first]), weight=weight(n_unseen, first))
    return out


def sample(P, Q, bias, indptr, indices, users, pos, N, margin, seed, offset=0, accept=None, alias=None, lists=None):
    """The model of bpr_sample_warp on static tables: (items int32 [n], tries int32 [n], x_pos, x_neg float64 [n],
    undecided bool [n], eps float64 [n], accepted int [n])."""
    n = len(users)
    items, tries = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xp, xn, eps = np.zeros(n), np.zeros(n), np.zeros(n)
    und, acc = np.zeros(n, bool), np.zeros(n, np.int64)
    seen_of = {}
    for b, u in enumerate(users.tolist()):
        if u not in seen_of:
            seen_of[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
        r = draw(seed, offset + b, u, int(pos[b]), N, margin, P, Q, bias, indptr, indices, accept, alias, seen_of[u],
                 None if lists is None else lists[b])
        items[b], tries[b], xp[b], xn[b] = r["item"], r["tries"], r["x_pos"], r["x_neg"]
        und[b], eps[b], acc[b] = r["undecided"], r["eps"], r["accepted"]
    return items, tries, xp, xn, und, eps, acc


def step(P, Q, bias, u, i, j, L, lr, alphas):
    """oracle.step_sgd_sparse on the one triple with the weight L in the place of sigma(-x): the oracle's update is
    -lr (sigma g + alpha r) (g the BPR gradient, r the rows), so calling it with lr L / sigma and alpha sigma / L
    gives -lr (L g + alpha r) — the substitution, in the oracle's own arithmetic.  sigma comes from the oracle's
    logits (a call with lr = 0).  L = 0: the L2 terms alone, in float64.  In place; returns the L2 term."""
    us, ps, ns = (np.array([v], np.int32) for v in (u, i, j))
    p, qi, qj = (r.astype(np.float64) for r in (P[u], Q[i], Q[j]))
    reg = 0.5 * (alphas[1] * qi @ qi + alphas[2] * qj @ qj + alphas[0] * p @ p)
    if L == 0.0:
        P[u] = (p - lr * alphas[0] * p).astype(np.float32)
        if i == j:
            Q[i] = (qi - lr * (alphas[1] + alphas[2]) * qi).astype(np.float32)
        else:
            Q[i] = (qi - lr * alphas[1] * qi).astype(np.float32)
            Q[j] = (qj - lr * alphas[2] * qj).astype(np.float32)
        return reg
    lp, ln, _ = oracle.step_sgd_sparse(P, Q, bias, us, ps, ns, 0.0, (0.0, 0.0, 0.0))
    sig = 1.0 / (1.0 + math.exp(float(lp[0] - ln[0])))
    oracle.step_sgd_sparse(P, Q, bias, us, ps, ns, lr * L / sig, tuple(a * sig / L for a in alphas))
    return reg


def train_sequential(P, Q, bias, indptr, indices, users, pos, N, margin, lr, alphas, seed, offset=0):
    """One triple at a time: the draw from the live rows, then `step` — or nothing at all for a skipped triple.  P, Q,
    bias are updated in place.  Returns (negatives int32 [n] (-1 = skipped), tries int32 [n], undecided bool [n],
    scalars float64 [4]: sum L (margin - x_i + x_k), the L2 term, sum |x_i - x_k|, stepped triples)."""
    n = len(users)
    neg, tries, und = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, bool)
    sc = np.zeros(4)
    seen_of = {}
    for t in range(n):
        u = int(users[t])
        if u not in seen_of:
            seen_of[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
        r = draw(seed, offset + t, u, int(pos[t]), N, margin, P, Q, bias, indptr, indices, seen=seen_of[u])
        neg[t], tries[t], und[t] = r["item"], r["tries"], r["undecided"]
        if r["item"] < 0:
            continue
        x = r["x_pos"] - r["x_neg"]
        sc += (r["weight"] * (margin - x), step(P, Q, bias, u, int(pos[t]), r["item"], r["weight"], lr, alphas),
               abs(x), 1.0)
    return neg, tries, und, sc


def tries_pmf(v, N):
    """P(tries = k), k = 1 .. N, and P(skipped), for candidates drawn uniformly with replacement from unseen items of
    which the share v violates: the truncated geometric (1 - v)^(k-1) v and (1 - v)^N."""
    k = np.arange(1, N + 1, dtype=np.float64)
    return (1.0 - v) ** (k - 1) * v, (1.0 - v) ** N
