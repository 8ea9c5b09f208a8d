"""numpy model of the re-ranking contract (`bpr_rerank_rows`, revisit_bpr/rerank.py) — TEST INFRASTRUCTURE ONLY.
Brute force, plain loops, the score matrix S as an input (as rank_model.rank_rows takes it), so nothing here comes
from the code under test.  Pinned against an independent torch statement by tests/test_rerank_cpu.py.

The contract it restates:
  eligibility  a candidate c of row r (user u) is eligible iff 0 < c < I and c is not in u's row of the seen CSR;
  cand_scores  S[u, c] for an eligible candidate, -inf otherwise, aligned with the candidate list;
  order        score descending, ties by ascending id;
  duplicates   the list is a multiset: an id listed m times is m candidates and may come back m times, adjacent;
  padding      a row with fewer than k eligible candidates ends in id -1 / score -inf."""
import numpy as np


def eligible(I, u, c, indptr, indices):
    if not 0 < c < I:
        return False
    if indptr is None:
        return True
    row = indices[indptr[u]:indptr[u + 1]]
    return not bool((row == c).any())


def rerank_rows(S, users, cptr, citems, k, indptr=None, indices=None):
    """S [U, I] float32.  cptr None: `citems` is the one list of every row (cand_scores is then [n, C]).
    Returns (items [n, k] int32, scores [n, k] float32, cand_scores float32)."""
    I, n = S.shape[1], len(users)
    items = np.full((n, k), -1, np.int32)
    scores = np.full((n, k), -np.inf, np.float32)
    shared = cptr is None
    cand = np.full((n, len(citems)) if shared else len(citems), -np.inf, np.float32)
    for r, u in enumerate(users):
        lo, hi = (0, len(citems)) if shared else (int(cptr[r]), int(cptr[r + 1]))
        live = []
        for p in range(lo, hi):
            c = int(citems[p])
            if eligible(I, u, c, indptr, indices):
                s = S[u, c]
                if shared:
                    cand[r, p] = s
                else:
                    cand[p] = s
                live.append((-float(s), c))
        live.sort()  # (−score, id): copies of one id are equal pairs and stay adjacent
        for j, (ms, c) in enumerate(live[:k]):
            items[r, j], scores[r, j] = c, np.float32(-ms)
    return items, scores, cand
