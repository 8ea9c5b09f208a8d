"""A control-flow model of `k_foldin_items` (revisit-bpr_amd/csrc/bpr_foldin_items.hip) in plain numpy, and the
definition it must reproduce, in the manner of tests/foldin_model.py.  `restate` is the definition of
include/bprcore.h (bpr_fold_in_item_rows), triple by triple.  `pipeline` walks the same rows the way the kernel does:
`groups` groups in lockstep, rows by ticket from `order`, and per group four rings of `pf` slots — ids (triple
c + 3 pf), bounds (c + 2 pf), sample (c + pf), update (c) — with a row entering at slot 0 and draining through 3 pf
further steps.  Both use the same float64 arithmetic per triple, so they agree BITWISE exactly when the pipeline applies
the same triples in the same order with the same operands.

Negatives: an int array (given, entry t) or a callable `draw(u, seen_row, t)` (sampled: a pure function of the user's
seen row and the counter, as the device sampler is); `seen` is (indptr, indices) of the users or None.
(tests/test_foldin_items_cpu.py)"""
import numpy as np

NO_TRIPLE, BAD_USER = -2, -1


def step(q, b, pu, qj, bj, lr, reg):
    """One update of (q, b) in place; returns the new b."""
    w = 1.0 / (1.0 + np.exp(float(np.cumsum(pu * (q - qj))[-1]) + (b - bj)))
    q += -lr * (-w * pu + reg * q)
    return b + lr * w


def seen_row(seen, u):
    if seen is None:
        return np.zeros(0, np.int64)
    return seen[1][int(seen[0][u]):int(seen[0][u + 1])]


def restate(P, Q, bias, indptr, users, neg, Q0, b0, epochs, lr, reg, seen=None):
    """(Q_new, b_new, negatives: the draws when sampled, 0 for a user out of range).  `bias` None: no bias term
    (b_new stays b0)."""
    P, Q, Qn = P.astype(np.float64), Q.astype(np.float64), Q0.astype(np.float64).copy()
    bn = np.asarray(b0, np.float64).copy()
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    used = np.zeros(epochs * nnz, np.int64)
    for r in range(len(indptr) - 1):
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                t, u = e * nnz + k - base, int(users[k])
                if not 0 <= u < len(P):
                    continue
                j = int(neg(u, seen_row(seen, u), t)) if callable(neg) else int(neg[t])
                used[t] = j
                if not 1 <= j < len(Q):
                    continue
                if bias is None:
                    step(Qn[r], 0.0, P[u], Q[j], 0.0, lr, reg)
                else:
                    bn[r] = step(Qn[r], bn[r], P[u], Q[j], float(bias[j]), lr, reg)
    return Qn, bn, used


class _Group:
    def __init__(self, pf):
        self.finished, self.row, self.lo, self.len, self.total, self.left = False, -1, 0, 0, 0, 0
        self.fc = self.fe = self.fk = 0
        self.q, self.b = None, 0.0
        self.fu, self.fx = [NO_TRIPLE] * pf, [0] * pf  # ids
        self.bu, self.bx = [NO_TRIPLE] * pf, [0] * pf  # bounds
        self.srow, self.pa = [None] * pf, [None] * pf
        self.un = [0] * pf  # sample
        self.pu, self.qj, self.bj = [None] * pf, [None] * pf, [0.0] * pf


def pipeline(P, Q, bias, indptr, users, neg, Q0, b0, epochs, lr, reg, pf, groups, order=None, seen=None):
    """The kernel's loop, statement for statement (one wave: `groups` groups share every step).  Returns
    (Q_new, b_new, negatives written (sampled only), steps)."""
    m, U, I = len(indptr) - 1, len(P), len(Q)
    P, Q, Qn = P.astype(np.float64), Q.astype(np.float64), Q0.astype(np.float64).copy()
    bn = np.asarray(b0, np.float64).copy()
    base0, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    sampled = callable(neg)
    used = np.zeros(epochs * nnz, np.int64)
    ticket = 0
    gs = [_Group(pf) for _ in range(groups)]
    steps = 0
    while True:
        while any(not g.finished and g.left == 0 for g in gs):  # ring slot 0: write back, next ticket
            for g in gs:
                if g.finished or g.left != 0:
                    continue
                if g.row >= 0:
                    Qn[g.row] = g.q
                    if bias is not None:
                        bn[g.row] = g.b
                tk, ticket = ticket, ticket + 1
                g.row, g.len, g.total, g.left = -1, 0, 0, 0
                if tk >= m:
                    g.finished = True
                    continue
                r = int(order[tk]) if order is not None else tk
                if 0 <= r < m:
                    g.row, g.lo = r, int(indptr[r])
                    g.len = int(indptr[r + 1]) - g.lo
                    g.total = epochs * g.len
                    g.left = g.total + 3 * pf if g.total > 0 else 0
                    g.fc = g.fe = g.fk = 0
                    g.q = Qn[r].copy()
                    g.b = float(bn[r]) if bias is not None else 0.0
        if all(g.finished for g in gs):
            return Qn, bn, used, steps
        for s in range(pf):
            steps += 1
            for g in gs:
                if g.un[s] != 0:  # update
                    nb = step(g.q, g.b, g.pu[s], g.qj[s], g.bj[s], lr, reg)
                    g.b = nb if bias is not None else g.b
                u = g.bu[s]  # sample
                j = 0
                if sampled:
                    if u >= 0 and len(g.srow[s]) < I - 1:
                        j = int(neg(u, g.srow[s], g.bx[s]))
                    if u != NO_TRIPLE:
                        used[g.bx[s]] = j
                else:
                    j = g.bx[s]
                j = j if u >= 0 else 0
                g.un[s] = j
                g.pu[s] = g.pa[s]
                if j != 0:
                    g.qj[s], g.bj[s] = Q[j].copy(), (float(bias[j]) if bias is not None else 0.0)
                u = g.fu[s]  # bounds
                g.bu[s], g.bx[s] = u, g.fx[s]
                if u >= 0:
                    g.srow[s] = seen_row(seen, u)
                    g.pa[s] = P[u].copy()
                valid = not g.finished and g.fc < g.total  # ids
                t = g.fe * nnz + (g.lo - base0) + g.fk
                u = int(users[g.lo + g.fk]) if valid else 0
                ok = valid and 0 <= u < U
                if sampled:
                    x = t
                else:
                    x = int(neg[t]) if valid else 0
                    ok = ok and 1 <= x < I
                    x = x if ok else 0
                g.fu[s] = u if ok else (BAD_USER if valid else NO_TRIPLE)
                g.fx[s] = x
                if valid:
                    g.fc += 1
                    g.fk += 1
                    if g.fk == g.len:
                        g.fk, g.fe = 0, g.fe + 1
                g.left -= 1 if g.left > 0 else 0
