"""The definition of `bpr_fold_in_item_rows_roles` (include/bprcore.h) in plain numpy, and a control-flow model of
its kernel (`k_foldin_items_roles`, revisit-bpr_amd/csrc/bpr_foldin_items_roles.hip), in the manner of
tests/foldin_items_model.py.

The definition: `schedule` (which steps of a pass are negative-role steps), `role_draw` (the Philox draw of a
negative-role step's training interaction), `step` (both updates) and `restate`, which applies them step by step.
`pipeline` walks the same rows the way the kernel does: `groups` groups in lockstep, rows by ticket from `order`, per
group four rings of `pf` slots — ids (step c + 3 pf; the schedule is walked with the kernel's accumulator, not with the
definition's divisions), bounds (c + 2 pf; a negative-role step's attempt is accepted here), sample (c + pf), update
(c) — a row entering at slot 0 and draining through 3 pf further steps.  Both use the same arithmetic per step, so they
agree BITWISE exactly when the pipeline applies the same steps in the same order with the same operands.

Positive-role negatives: an int array (given, entry t) or a callable `draw(u, seen_row, t)` (sampled), `seen` =
(indptr, indices) of the users or None — as in tests/foldin_items_model.py.
(tests/test_foldin_items_roles_cpu.py, tests/test_gpu_foldin_items_roles.py)"""
import functools

import numpy as np

NO_TRIPLE, BAD_USER = -2, -1
ATTEMPTS, PURPOSE_ROLE = 16, 2
M32 = 0xFFFFFFFF


def schedule(L, R):
    """[(negative role?, k or rho)] for the L + R steps of a pass: step s is a negative-role step iff
    floor((s + 1) R / (L + R)) > floor(s R / (L + R)); rho = floor(s R / (L + R)), k = s - rho."""
    n = L + R
    out = []
    for s in range(n):
        rho = s * R // n
        role = (s + 1) * R // n > rho
        out.append((role, rho if role else s - rho))
    return out


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11): counter words c[0..3], key words k[0..1] -> four 32-bit words."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=None)
def role_words(seed, counter):
    """The 16 words w_0 .. w_15 of a negative-role step: word a & 3 of the block with counter words
    (lo32(counter), hi32(counter), a >> 2, 2) under the key (lo32(seed), hi32(seed))."""
    counter &= 0xFFFFFFFFFFFFFFFF
    words = []
    for block in range(ATTEMPTS // 4):
        words += philox4x32_10((counter & M32, counter >> 32, block, PURPOSE_ROLE), (seed & M32, (seed >> 32) & M32))
    return tuple(words)


def role_draw(train, U, I, audience, seed, counter):
    """Index into the training arrays of the first accepted attempt, or -1.  `audience`: the row's sorted users."""
    tu, ti = train
    for w in role_words(seed, counter):
        tau = (w * len(tu)) >> 32
        u, i = int(tu[tau]), int(ti[tau])
        if 0 <= u < U and 1 <= i < I:
            at = int(np.searchsorted(audience, u))
            if at == len(audience) or int(audience[at]) != u:
                return tau
    return -1


def step(q, b, pu, qo, bo, lr, reg, role, f=np.float64):
    """One update of (q, b) in place in the number format `f`; returns the new b.  `role`: negative-role step (the
    other item `qo`, `bo` is the training interaction's), else positive-role step (it is the negative).  The dot is
    a sequential chain (cumsum adds left to right)."""
    one = f(1)
    if role:
        x = f(np.cumsum(pu * (qo - q), dtype=f)[-1] + f(bo - b))
        w = f(one / f(one + np.exp(x)))
        q += f(-lr) * (w * pu + reg * q)
        return f(b - f(lr * w))
    x = f(np.cumsum(pu * (q - qo), dtype=f)[-1] + f(b - bo))
    w = f(one / f(one + np.exp(x)))
    q += f(-lr) * (f(-w) * pu + reg * q)
    return f(b + f(lr * w))


def seen_row(seen, u):
    if seen is None:
        return np.zeros(0, np.int64)
    return seen[1][int(seen[0][u]):int(seen[0][u + 1])]


def _formats(P, Q, bias, Q0, b0, lr, reg, f):
    bias = None if bias is None else np.asarray(bias).astype(f)
    return (P.astype(f), Q.astype(f), bias, Q0.astype(f).copy(), np.asarray(b0).astype(f).copy(), f(np.float32(lr)),
            f(np.float32(reg)))


def restate(P, Q, bias, indptr, users, neg, Q0, b0, epochs, lr, reg, R, train, seed, offset, seen=None, rows=None,
            f=np.float64):
    """The definition, step by step.  Returns (Q_new, b_new, negatives of the positive-role steps: the draws when
    sampled, 0 for a user out of range; role_out).  `bias` None: no bias term (b_new stays b0).  `rows`: the rows to
    walk (default all; the others keep their values and their role_out entries stay -7)."""
    P, Q, bias, Qn, bn, lr, reg = _formats(P, Q, bias, Q0, b0, lr, reg, f)
    m = len(indptr) - 1
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    used = np.zeros(epochs * nnz, np.int64)
    roles = np.full(epochs * m * R, -7, np.int64)
    for r in (range(m) if rows is None else rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        audience = users[lo:hi]
        b = f(0) if bias is None else bn[r]
        for e in range(epochs):
            for role, at in schedule(hi - lo, R):
                if role:
                    g = (e * m + r) * R + at
                    tau = role_draw(train, len(P), len(Q), audience, seed, offset + g)
                    roles[g] = tau
                    if tau < 0:
                        continue
                    u, o = int(train[0][tau]), int(train[1][tau])
                else:
                    t, u = e * nnz + lo + at - base, int(users[lo + at])
                    if not 0 <= u < len(P):
                        continue
                    o = int(neg(u, seen_row(seen, u), t)) if callable(neg) else int(neg[t])
                    used[t] = o
                    if not 1 <= o < len(Q):
                        continue
                nb = step(Qn[r], b, P[u], Q[o], f(0) if bias is None else bias[o], lr, reg, role, f)
                b = b if bias is None else nb
        if bias is not None:
            bn[r] = b
    return Qn, bn, used, roles


class _Group:
    def __init__(self, pf):
        self.finished, self.row, self.lo, self.len, self.total, self.left = False, -1, 0, 0, 0, 0
        self.fc = self.fe = self.fk = self.fr = self.facc = 0
        self.q, self.b = None, 0.0
        self.fu, self.fx = [NO_TRIPLE] * pf, [0] * pf  # ids (negative role: one entry per attempt)
        self.ft, self.fg = [0] * pf, [-1] * pf
        self.bu, self.bx, self.bk = [NO_TRIPLE] * pf, [0] * pf, [False] * pf  # bounds
        self.srow, self.pa = [None] * pf, [None] * pf
        self.un, self.uk = [0] * pf, [False] * pf  # sample
        self.pu, self.qo, self.bo = [None] * pf, [None] * pf, [0.0] * pf


def pipeline(P, Q, bias, indptr, users, neg, Q0, b0, epochs, lr, reg, R, train, seed, offset, pf, groups, order=None,
             seen=None, f=np.float64):
    """The kernel's loop, statement for statement (one wave: `groups` groups share every step).  Returns
    (Q_new, b_new, negatives written (sampled only), role_out, steps)."""
    m, U, I = len(indptr) - 1, len(P), len(Q)
    P, Q, bias, Qn, bn, lr, reg = _formats(P, Q, bias, Q0, b0, lr, reg, f)
    base0, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    sampled = callable(neg)
    used = np.zeros(epochs * nnz, np.int64)
    roles = np.full(epochs * m * R, -7, np.int64)
    T = len(train[0]) if R else 0
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
                    g.total = epochs * (g.len + R)
                    g.left = g.total + 3 * pf if g.total > 0 else 0
                    g.fc = g.fe = g.fk = g.fr = g.facc = 0
                    g.q = Qn[r].copy()
                    g.b = bn[r] if bias is not None else f(0)
        if all(g.finished for g in gs):
            return Qn, bn, used, roles, steps
        for s in range(pf):
            steps += 1
            for g in gs:
                if g.un[s] != 0:  # update
                    nb = step(g.q, g.b, g.pu[s], g.qo[s], g.bo[s], lr, reg, g.uk[s], f)
                    g.b = nb if bias is not None else g.b
                u, role = g.bu[s], g.bk[s]  # sample
                j = 0
                if sampled:
                    if u >= 0 and not role and len(g.srow[s]) < I - 1:
                        j = int(neg(u, g.srow[s], g.bx[s]))
                    if u != NO_TRIPLE and not role:
                        used[g.bx[s]] = j
                    j = g.bx[s] if role else j
                else:
                    j = g.bx[s]
                j = j if u >= 0 else 0
                g.un[s], g.uk[s] = j, role
                g.pu[s] = g.pa[s]
                if j != 0:
                    g.qo[s], g.bo[s] = Q[j].copy(), (bias[j] if bias is not None else f(0))
                gi = g.fg[s]  # bounds
                role = gi >= 0
                u, x = g.fu[s], g.fx[s]
                if role:
                    audience = users[g.lo:g.lo + g.len]
                    ok = [a for a in range(ATTEMPTS) if 0 <= u[a] < U and 1 <= x[a] < I
                          and u[a] not in set(int(v) for v in audience)]
                    roles[gi] = g.ft[s][ok[0]] if ok else -1
                    u, x = (u[ok[0]], x[ok[0]]) if ok else (BAD_USER, 0)
                g.bu[s], g.bx[s], g.bk[s] = u, x, role
                if u >= 0:
                    if not role:
                        g.srow[s] = seen_row(seen, u)
                    g.pa[s] = P[u].copy()
                valid = not g.finished and g.fc < g.total  # ids
                n = g.len + R
                role = valid and g.facc + R >= n
                posv = valid and not role
                t = g.fe * nnz + (g.lo - base0) + g.fk
                u = int(users[g.lo + g.fk]) if posv else 0
                ok = posv and 0 <= u < U
                if sampled:
                    x = t
                else:
                    x = int(neg[t]) if posv else 0
                    ok = ok and 1 <= x < I
                    x = x if ok else 0
                u = u if ok else (BAD_USER if valid else NO_TRIPLE)
                tau, gi = 0, -1
                if role:
                    gi = (g.fe * m + g.row) * R + g.fr
                    tau = [(w * T) >> 32 for w in role_words(seed, offset + gi)]
                    u, x = [int(train[0][a]) for a in tau], [int(train[1][a]) for a in tau]
                g.fu[s], g.fx[s], g.ft[s], g.fg[s] = u, x, tau, gi
                if valid:
                    g.fc += 1
                    g.facc += R
                    if role:
                        g.facc -= n
                        g.fr += 1
                    else:
                        g.fk += 1
                    if g.fk + g.fr == n:
                        g.fk = g.fr = g.facc = 0
                        g.fe += 1
                g.left -= 1 if g.left > 0 else 0
