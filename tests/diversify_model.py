"""Brute-force numpy model of `bpr_diversify_rows` (include/bprcore.h): test infrastructure, nothing of it comes from
the code under test.  `sim_matrix` restates the similarity in float32 steps, `diversify_rows` is the greedy loop with
the tie rule, the rows of a call advancing together a step at a time."""
import numpy as np

from chain_model import chain_scores

F = np.float32


def chain_dot(A, B):
    """dot(a, b) for every pair of rows of A [m, d] and B [p, d]: one float32 accumulator from +0, one fused
    multiply-add per feature in k_topk's order (per 8 features 0, 4, 1, 5, 2, 6, 3, 7), every chunk of 32 run to its
    end over zeros.  There is one host model of that chain, tests/chain_model.py, whose fma is correctly rounded
    (tests/test_chain_model_cpu.py holds it to exact rational arithmetic); this is it."""
    return chain_scores(A, B)


def sim_matrix(Q, metric):
    """sim(a, b) for every pair of rows of Q, float32 [I, I]: "dot", or "cosine" = dot * (rn(a) * rn(b)) with
    rn(v) = 1 / sqrt(dot(v, v)) in correctly rounded float32 steps; a row with !(dot(v, v) > 0) has similarity 0 to
    everything."""
    G = chain_dot(Q, Q)
    if metric == "dot":
        return G
    assert metric == "cosine"
    ss = np.diagonal(G).astype(F)
    good = ss > 0
    with np.errstate(all="ignore"):
        rn = np.where(good, F(1) / np.sqrt(np.where(good, ss, F(1)), dtype=F), F(0)).astype(F)
        S = (G * (rn[:, None] * rn[None, :]).astype(F)).astype(F)
    S[~good, :] = 0
    S[:, ~good] = 0
    return S


def diversify_rows(S, cand_items, cand_scores, k, lam, scale="none"):
    """(items [n, k] int32, scores [n, k] float32, mmr [n, k] float32, ties): greedy MMR of every row over the
    similarity matrix S [I, I]; the rows advance together, a step at a time.  `ties` counts the steps at which the
    largest objective was shared by more than one unpicked candidate, i.e. the steps the tie rule decided."""
    S = np.asarray(S, F)
    I = S.shape[0]
    ci = np.atleast_2d(np.asarray(cand_items, np.int32)).astype(np.int64)
    cs = np.atleast_2d(np.asarray(cand_scores, F))
    n = ci.shape[0]
    lam = F(lam)
    oml = F(1) - lam
    items = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, F)
    mmr = np.full((n, k), -np.inf, F)
    ties = 0
    with np.errstate(all="ignore"):
        left = (ci > 0) & (ci < I) & np.isfinite(cs)  # eligible and not picked yet
        ids = np.where(left, ci, 0)
        rel = np.where(left, cs, F(0)).astype(F)
        relp = rel
        if scale == "minmax":
            lo = np.where(left, cs, F(np.inf)).min(1, keepdims=True).astype(F)
            hi = np.where(left, cs, F(-np.inf)).max(1, keepdims=True).astype(F)
            relp = np.where(hi == lo, F(0), ((rel - lo).astype(F) / (hi - lo).astype(F)).astype(F)).astype(F)
        else:
            assert scale == "none"
        m = np.zeros(ci.shape, F)
        for step in range(k):
            rows = np.nonzero(left.any(1))[0]
            if not len(rows):
                break
            v = ((lam * relp).astype(F) - (oml * m).astype(F)).astype(F)  # three roundings
            v = np.where(np.isnan(v), F(-np.inf), v)
            # the largest v; among those the largest relevance; among those the smallest id; then the first position
            sel = left & (v == np.where(left, v, F(-np.inf)).max(1, keepdims=True))
            ties += int((sel.sum(1) > 1).sum())
            sel &= rel == np.where(sel, rel, F(-np.inf)).max(1, keepdims=True)
            sel &= ids == np.where(sel, ids, np.int64(2) ** 40).min(1, keepdims=True)
            best = sel.argmax(1)
            items[rows, step] = ids[rows, best[rows]]
            scores[rows, step] = rel[rows, best[rows]]
            mmr[rows, step] = v[rows, best[rows]]
            left[rows, best[rows]] = False
            sim = S[ids, ids[np.arange(n), best][:, None]]
            m = sim.copy() if step == 0 else np.where(sim > m, sim, m)
    return items, scores, mmr, ties
