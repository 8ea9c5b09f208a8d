"""numpy model of the ranking contract (`bpr_rank_rows`, revisit_bpr/ranks.py) and of the metric formulas of
`evaluation.evaluate_ranked` — TEST INFRASTRUCTURE ONLY.  Brute force over the eligible items; plain loops.

Pinned against oracle/metrics_np.py and the torch metric classes on a dense example by tests/test_rank_cpu.py, so
that the GPU tests (tests/test_gpu_rank.py) have a yardstick that does not come from the code under test."""
import math

import numpy as np


def eligible(I, u, indptr, indices):
    ok = np.ones(I, bool)
    ok[0] = False
    if indptr is not None:
        ok[indices[indptr[u]:indptr[u + 1]]] = False
    return ok


def rank_rows(S, users, tptr, titems, indptr=None, indices=None):
    """S [U, I] float32 scores.  Returns (rank, not_below, score) aligned with titems."""
    I = S.shape[1]
    ids = np.arange(I)
    rank = np.full(len(titems), -1, np.int32)
    not_below = np.full(len(titems), -1, np.int32)
    score = np.full(len(titems), -np.inf, np.float32)
    for r, u in enumerate(users):
        ok = eligible(I, u, indptr, indices)
        for p in range(tptr[r], tptr[r + 1]):
            t = titems[p]
            if not (0 <= t < I) or not ok[t]:
                continue
            others = ok & (ids != t)
            s, st = S[u], S[u, t]
            rank[p] = int((others & ((s > st) | ((s == st) & (ids < t)))).sum())
            not_below[p] = int((others & (s >= st)).sum())
            score[p] = st
    return rank, not_below, score


def user_metrics(rank, not_below, score, tptr, titems, I, n_seen, ks, masked_negatives=True):
    """Per-user values by evaluate_ranked's keys (ndcg / recall / precision / map @k, mrr, auc), float64 [E]."""
    E = len(tptr) - 1
    out = {f"{m}@{k}": np.zeros(E) for k in ks for m in ("ndcg", "recall", "precision", "map")}
    out["mrr"], out["auc"] = np.zeros(E), np.zeros(E)
    for e in range(E):
        n_pos = int(tptr[e + 1] - tptr[e])
        listed, got, in_range, out_of_play = set(), [], 0, 0
        for p in range(tptr[e], tptr[e + 1]):
            t = int(titems[p])
            if t in listed:  # a target counts once
                continue
            listed.add(t)
            in_range += 0 <= t < I
            if rank[p] >= 0:
                got.append((int(rank[p]), int(not_below[p]), float(score[p])))
            elif 0 <= t < I:
                out_of_play += 1
        got.sort()
        for k in ks:
            kk = min(k, I)
            top = [g for g in got if g[0] < kk]
            ideal = sum(1.0 / math.log2(i + 2.0) for i in range(min(n_pos, kk)))
            out[f"ndcg@{k}"][e] = sum(1.0 / math.log2(g[0] + 2.0) for g in top) / ideal if ideal > 0 else 0.0
            out[f"recall@{k}"][e] = len(top) / n_pos if n_pos else 0.0
            out[f"precision@{k}"][e] = len(top) / kk
            out[f"map@{k}"][e] = sum((c + 1) / (g[0] + 1) for c, g in enumerate(top)) / min(n_pos, kk) if n_pos else 0.0
        out["mrr"][e] = 1.0 / (got[0][0] + 1) if got else 0.0
        n_elig = I - 1 - int(n_seen[e])
        wins = 0
        for _, nb, s in got:
            below = n_elig - 1 - nb - sum(1 for g in got if g[2] < s)  # eligible non-targets strictly below
            if masked_negatives and s > -1e13:
                below += int(n_seen[e]) + 1 - out_of_play  # item 0 and the seen items that are not positives
            wins += below
        T = in_range if masked_negatives else len(got)
        n_neg = I - T if masked_negatives else n_elig - len(got)
        out["auc"][e] = wins / (T * n_neg) if T * n_neg else np.nan
    return out
