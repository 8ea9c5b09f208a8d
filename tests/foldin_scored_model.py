"""Fold-in with scored negatives (`bpr_fold_in_rows_scored`, revisit-bpr_amd/csrc/bpr_foldin_scored.hip) in plain numpy:
the definition of include/bprcore.h restated on the models of its parts, and a control-flow model of the kernel in the
manner of tests/foldin_adaptive_model.py.  Shared by tests/test_foldin_scored_cpu.py and
tests/test_gpu_foldin_scored.py; nothing here needs a GPU.

`restate` is the definition: row by row, epoch by epoch, position by position; the draw of a triple is
dynamic_model.pick / warp_model.draw on the row as it stands (float64), the step is foldin_model.step (with the bias
term where there is a bias) or the WARP step with warp_model.weight's L.  It also says which triples the fp32 kernel
may decide differently (dynamic_model's `decided`, warp_model's `undecided`).

`flow` / `pipeline`: the sampler is abstract — `sampler(t, p, r)` -> (j, L): any pure function of the triple index,
the row's state just before the triple and the row; j < 1 skips the triple, L None takes BPR's step and a number the
WARP step.  `flow` asks it in the definition's order; `pipeline` walks the rows the way the kernel does: `groups`
groups in lockstep, rows by ticket from `order`, per group a ring of `pf` slots holding the positive (and, `ring_rows`,
its row: BPR_NEG_DYNAMIC) of the triples fetched ahead; a step consumes the triple fetched pf steps ago (draw ->
update) and fetches the next.  A group with nothing to consume takes a DUMMY draw whenever another group of the wave
draws (counted apart: it must change nothing).  Every loop carries a cap that fails the test instead of spinning."""
import numpy as np

import dynamic_model as dm
import warp_model as wm
from foldin_model import step


def bpr_step(p, qi, qj, bi, bj, lr, reg):
    """foldin_model.step, with the bias term of x where there is one."""
    if bi == 0.0 and bj == 0.0:
        return step(p, qi, qj, lr, reg)
    diff = qi - qj
    w = 1.0 / (1.0 + np.exp(float(np.cumsum(p * diff)[-1]) + (bi - bj)))
    p += -lr * (-w * diff + reg * p)


def warp_step(p, qi, qj, L, lr, reg):
    p += -lr * (-L * (qi - qj) + reg * p)


def restate(kind, Q, bias, indptr, items, P0, epochs, lr, reg, K, margin, seed, offset):
    """-> (rows float64, negatives int32, tries int32, undecided bool), the last three [epochs * nnz]."""
    I, n = len(Q), len(indptr) - 1
    Qd, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    b = np.zeros(I) if bias is None else bias.astype(np.float64)
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    neg, tries, und = (np.zeros(epochs * nnz, dt) for dt in (np.int32, np.int32, bool))
    for r in range(n):
        seen, p = set(items[indptr[r]:indptr[r + 1]].tolist()), P[r]
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                t, i = e * nnz + k - base, int(items[k])
                i = i if 1 <= i < I else 0
                if kind == "dynamic":
                    dr = dm.pick(seed, offset + t, 0, K, p[None], Q, bias, None, None, seen=seen)
                    j, und[t] = dr["item"], not dr["decided"]
                    if j >= 1 and i >= 1:
                        bpr_step(p, Qd[i], Qd[j], b[i], b[j], lr, reg)
                else:
                    dr = wm.draw(seed, offset + t, 0, i, K, margin, p[None], Q, bias, None, None, seen=seen)
                    j, tries[t], und[t] = dr["item"], dr["tries"], dr["undecided"]
                    if j >= 1 and i >= 1:
                        warp_step(p, Qd[i], Qd[j], dr["weight"], lr, reg)
                neg[t] = j
    return P, neg, tries, und


# ---- the control flow ------------------------------------------------------------------------------------------------
def apply(p, qi, qj, j, L, lr, reg):
    if j >= 1:
        if L is None:
            step(p, qi, qj, lr, reg)
        else:
            warp_step(p, qi, qj, L, lr, reg)


def flow(Q, indptr, items, P0, epochs, lr, reg, sampler):
    """-> (final rows, log of (t, row, state before t) in the order the definition asks the sampler)."""
    Q, P = Q.astype(np.float64), P0.astype(np.float64).copy()
    base, nnz = int(indptr[0]), int(indptr[-1] - indptr[0])
    log = []
    for r in range(len(indptr) - 1):
        for e in range(epochs):
            for k in range(int(indptr[r]), int(indptr[r + 1])):
                t = e * nnz + k - base
                log.append((t, r, P[r].copy()))
                j, L = sampler(t, P[r], r)
                i = int(items[k])
                if 1 <= i < len(Q):
                    apply(P[r], Q[i], Q[max(j, 0)], j, L, lr, reg)
    return P, log


class _Group:
    def __init__(self, pf):
        self.finished, self.row, self.lo, self.m, self.total, self.left = False, -1, 0, 0, 0, 0
        self.fc = self.fe = self.fj = self.ce = self.cj = 0
        self.p = None
        self.si, self.qi = [0] * pf, [None] * pf


def pipeline(Q, indptr, items, P0, epochs, lr, reg, sampler, pf, groups, order=None, ring_rows=True):
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
            if any(cv):  # the draw runs for the whole wave or not at all
                for g, c in zip(gs, cv):
                    if not c:
                        dummies += 1  # a dummy draw: its result is dropped, nothing of the group changes
                        continue
                    t = g.ce * nnz + (g.lo - base0) + g.cj
                    log.append((t, g.row, g.p.copy()))
                    j, L = sampler(t, g.p, g.row)  # sees every earlier update of the row
                    i = g.si[s]
                    if i != 0:
                        apply(g.p, g.qi[s] if ring_rows else Q[i], Q[max(j, 0)], j, L, lr, reg)
                    g.cj += 1
                    if g.cj == g.m:
                        g.cj, g.ce = 0, g.ce + 1
            for g in gs:  # fetch
                valid = not g.finished and g.fc < g.total
                i = int(items[g.lo + g.fj]) if valid else 0
                i = i if 1 <= i < len(Q) else 0
                g.si[s] = i
                if valid:
                    if ring_rows and i != 0:
                        g.qi[s] = Q[i].copy()
                    g.fc += 1
                    g.fj += 1
                    if g.fj == g.m:
                        g.fj, g.fe = 0, g.fe + 1
                g.left -= 1 if g.left > 0 else 0


# ---- the committed inputs of the GPU tests' free-running cases ----------------------------------------------------------
LR, REG, MARGIN, SEED, OFFSET = 0.05, 0.02, 1.0, 11, 1_000_003
# seeds of the free-running problems per (I, d, N), chosen on the CPU so that the model leaves NO triple of either kind
# undecided (tests/test_foldin_scored_cpu.py asserts it)
RUN_SEED = {(50, 8, 4): 0, (50, 33, 10): 0, (50, 128, 4): 0, (50, 300, 10): 0, (50, 1024, 4): 1}
RUN_EPOCHS = 2


def lengths(I):
    return [0, 1, 2, 3, 9, 17, 40, I - 2, I - 1]  # tests/test_gpu_foldin_adaptive.py: lengths


def problem(I, d, seed, bias=True):
    """Tables, histories and initial rows: scores of standard deviation 0.05, every second user's row scaled by 4.0 / 0.05
    so that there the positive's rank decides (tests/warp_cases.py: problem)."""
    rng = np.random.default_rng(100_000 * seed + 1000 * I + d)
    lens = lengths(I)
    rows = [np.sort(rng.choice(np.arange(1, I), size=k, replace=False)).astype(np.int32) for k in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    Q[0] = 0
    P0 = (rng.standard_normal((len(lens), d)) * (0.05 / d ** 0.5)).astype(np.float32)
    P0[1::2] *= np.float32(4.0 / 0.05)
    b = (rng.standard_normal(I) * 0.3).astype(np.float32) if bias else None
    return dict(I=I, d=d, lens=lens, rows=rows, indptr=indptr, items=items, Q=Q, b=b, P0=P0, n=len(lens),
                nnz=int(indptr[-1]))


_runs = {}


def run_model(kind, I, d, N):
    """`restate` of the free-running case (I, d, N), cached and read-only."""
    key = (kind, I, d, N)
    if key not in _runs:
        pr = problem(I, d, RUN_SEED[(I, d, N)])
        out = restate(kind, pr["Q"], pr["b"], pr["indptr"], pr["items"], pr["P0"], RUN_EPOCHS, LR, REG, N, MARGIN, SEED,
                      OFFSET)
        for a in out:
            a.setflags(write=False)
        _runs[key] = (pr, out)
    return _runs[key]
