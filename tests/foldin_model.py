"""A control-flow model of `k_foldin` (revisit-bpr_amd/csrc/bpr_foldin.hip) in plain numpy, and the definition it must
reproduce.  `restate` is the definition of include/bprcore.h, triple by triple.  `pipeline` walks the same rows the way
the kernel does: `groups` groups in lockstep, rows by ticket from `order`, and per group three rings of `pf` slots —
fetch (triple c + 2 pf), rows (triple c + pf), update (triple c) — with a row entering at slot 0 and draining through
2 pf further steps.  Both use the same float64 arithmetic per triple, so they agree BITWISE exactly when the pipeline
applies the same triples in the same order with the same operands: what the kernel's claim "the result does not
depend on the prefetch depth, the grid or the order" rests on.  (tests/test_foldin_model_cpu.py)"""
import numpy as np


def step(p, qi, qj, lr, reg):
    diff = qi - qj
    w = 1.0 / (1.0 + np.exp(float(np.cumsum(p * diff)[-1])))
    p += -lr * (-w * diff + reg * p)


def restate(Q, indptr, items, neg, P0, epochs, lr, reg):
    Q, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    for r in range(len(indptr) - 1):
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                j = int(neg[e * nnz + k - base])
                if j != 0:
                    step(P[r], Q[int(items[k])], Q[j], lr, reg)
    return P


class _Group:
    def __init__(self, pf):
        self.finished, self.row, self.lo, self.m, self.total, self.left = False, -1, 0, 0, 0, 0
        self.fc = self.fe = self.fj = 0
        self.p = None
        self.fi, self.fn, self.rn = [0] * pf, [0] * pf, [0] * pf
        self.qi, self.qj = [None] * pf, [None] * pf


def pipeline(Q, indptr, items, neg, P0, epochs, lr, reg, pf, groups, order=None):
    """The kernel's loop, statement for statement (one wave: `groups` groups share every step)."""
    n = len(indptr) - 1
    Q, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    base0, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    ticket = 0
    gs = [_Group(pf) for _ in range(groups)]
    steps = 0
    while True:
        while any(not g.finished and g.left == 0 for g in gs):  # ring slot 0: write back, next ticket
            for g in gs:
                if g.finished or g.left != 0:
                    continue
                if g.row >= 0:
                    P[g.row] = g.p
                tk, ticket = ticket, ticket + 1
                g.row, g.m, g.total, g.left = -1, 0, 0, 0
                if tk >= n:
                    g.finished = True
                    continue
                r = int(order[tk]) if order is not None else tk
                if 0 <= r < n:
                    g.row, g.lo = r, int(indptr[r])
                    g.m = int(indptr[r + 1]) - g.lo
                    g.total = epochs * g.m
                    g.left = g.total + 2 * pf if g.total > 0 else 0
                    g.fc = g.fe = g.fj = 0
                    g.p = P[r].copy()
        if all(g.finished for g in gs):
            return P, steps
        for s in range(pf):
            steps += 1
            for g in gs:
                if g.rn[s] != 0:  # update
                    step(g.p, g.qi[s], g.qj[s], lr, reg)
                i, j = g.fi[s], g.fn[s]  # rows
                g.rn[s] = j
                if j != 0:
                    g.qi[s], g.qj[s] = Q[i].copy(), Q[j].copy()
                valid = not g.finished and g.fc < g.total  # fetch
                i = j = 0
                if valid:
                    i = int(items[g.lo + g.fj])
                    j = int(neg[g.fe * nnz + (g.lo - base0) + g.fj])
                ok = valid and 1 <= i < len(Q) and 1 <= j < len(Q)
                g.fi[s], g.fn[s] = (i, j) if ok else (0, 0)
                if valid:
                    g.fc += 1
                    g.fj += 1
                    if g.fj == g.m:
                        g.fj, g.fe = 0, g.fe + 1
                g.left -= 1 if g.left > 0 else 0
