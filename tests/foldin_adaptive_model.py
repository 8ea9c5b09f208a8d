"""A control-flow model of `k_foldin_adaptive` (revisit-bpr_amd/csrc/bpr_foldin_adaptive.hip) in plain numpy, and the
definition it must reproduce, in the manner of tests/foldin_model.py.

The sampler is abstract here: `sampler(t, p, rnd, r)` is any pure function of the triple index, the row's state just
before the triple, the triple's randoms and the row; what matters is WHICH (t, state) pairs it is asked about, in
which order, and that the update it feeds lands before the next question.  `restate` is the definition: row by row,
epoch by epoch, position by position.  `pipeline` walks the same rows the way the kernel does: `groups` groups in
lockstep, rows by ticket from `order`, per group a ring of `pf` slots holding the positive, its row and the randoms
of the triples fetched ahead; a step consumes the triple fetched pf steps ago (draw -> negative's row -> update) and
fetches the next.  A group with nothing to consume takes a DUMMY draw whenever another group of the wave draws
(logged apart: it must change nothing).  Every loop carries a cap that fails the test instead of spinning."""
import numpy as np

from foldin_model import step


def randoms(t):
    """Stands for adaptive_randoms(seed, offset + t, ...): a function of the counter only."""
    return (t * 2654435761) % 1000003


def restate(Q, indptr, items, P0, epochs, lr, reg, sampler):
    """-> (final rows, log of (t, row, state before t) in the order the definition asks the sampler)."""
    Q, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    log = []
    for r in range(len(indptr) - 1):
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                t = e * nnz + k - base
                log.append((t, r, P[r].copy()))
                j = sampler(t, P[r], randoms(t), r)
                i = int(items[k])
                if j != 0 and 1 <= i < len(Q):
                    step(P[r], Q[i], Q[j], lr, reg)
    return P, log


class _Group:
    def __init__(self, pf):
        self.finished, self.row, self.lo, self.m, self.total, self.left = False, -1, 0, 0, 0, 0
        self.fc = self.fe = self.fj = self.ce = self.cj = 0
        self.p = None
        self.si, self.rnd, self.qi = [0] * pf, [None] * pf, [None] * pf


def pipeline(Q, indptr, items, P0, epochs, lr, reg, sampler, pf, groups, order=None):
    """The kernel's loop, statement for statement (one wave: `groups` groups share every step).
    -> (final rows, log of real draws, number of dummy draws, steps)."""
    n = len(indptr) - 1
    Q, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    base0, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    ticket, steps, dummies, log = 0, 0, 0, []
    gs = [_Group(pf) for _ in range(groups)]
    cap = epochs * nnz + (n + groups) * 2 * pf + 16  # every loop below ends long before this many trips
    outer = 0
    while True:
        outer += 1
        assert outer <= cap, "the outer loop does not end"
        trips = 0
        while any(not g.finished and g.left == 0 for g in gs):  # ring slot 0: write back, next ticket
            trips += 1
            assert trips <= n + groups + 1, "the ticket loop does not end"
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
                    g.left = g.total + pf if g.total > 0 else 0
                    g.fc = g.fe = g.fj = g.ce = g.cj = 0
                    g.p = P[r].copy()
        if all(g.finished for g in gs):
            assert ticket <= n + groups
            return P, log, dummies, steps
        for s in range(pf):
            steps += 1
            cv = [not g.finished and 0 < g.left <= g.total for g in gs]
            if any(cv):  # the sampler runs for the whole wave or not at all
                for g, c in zip(gs, cv):
                    if not c:
                        dummies += 1  # a dummy draw: its result is dropped, nothing of the group changes
                        continue
                    t = g.ce * nnz + (g.lo - base0) + g.cj
                    log.append((t, g.row, g.p.copy()))
                    j = sampler(t, g.p, g.rnd[s], g.row)  # sees every earlier update of the row
                    i = g.si[s]
                    if i != 0 and j != 0:
                        step(g.p, g.qi[s], Q[j], lr, reg)
                    g.cj += 1
                    if g.cj == g.m:
                        g.cj, g.ce = 0, g.ce + 1
            for g in gs:  # fetch
                valid = not g.finished and g.fc < g.total
                i = int(items[g.lo + g.fj]) if valid else 0
                i = i if 1 <= i < len(Q) else 0
                g.si[s] = i
                if valid:
                    g.rnd[s] = randoms(g.fe * nnz + (g.lo - base0) + g.fj)
                    if i != 0:
                        g.qi[s] = Q[i].copy()
                    g.fc += 1
                    g.fj += 1
                    if g.fj == g.m:
                        g.fj, g.fe = 0, g.fe + 1
                g.left -= 1 if g.left > 0 else 0
