"""A numpy restatement of the LDS tier's ALGORITHM (k_stream<..., LDSHOT>, revisit-bpr_amd/csrc/bpr_stream.h, and
its launch plan in csrc/bpr_stream_plan.h) — test infrastructure:

  * the partition of a launch's triples into runs: [0, tail1) in runs of L, [tail1, tail2) in runs of L / 2,
    [tail2, n) in runs of L / 4, every zone whole wave-loads of runs (`zones`, `runs_of`: the host's and the
    kernel's integer arithmetic side by side);
  * the deal of run pairs to persistent workgroups: ticket k of workgroup b = wave-load k x grid + b (`deal`);
  * the algebra of the private delta blocks: a workgroup reads a hot row as Q + its OWN delta, adds its updates to
    that delta, and the deltas are summed into the table at the launch's end; cold rows are updated in place
    (`run_launch`: plain SGD on one embedding dimension per row is enough to pin the algebra).

The HIP kernel itself is held to the oracle in tests/test_gpu_hotlds.py (`-m gpu`)."""
import numpy as np


def zones(n: int, L: int, gpw: int, tail_percent: int):
    """(tail1, tail2) as the launch plan computes them (csrc/bpr_stream_plan.h: plan_stream_lds; held to this
    function by tests/test_stream_plan_cpu.py): zones hold whole wave-loads of runs; what is left of the chunk
    past the last whole wave-load of full runs always goes in the shortest runs."""
    len2 = max(1, L // 2)
    wl = L * gpw
    t1 = int(n * (1.0 - tail_percent / 100.0)) // wl * wl
    t2 = t1 + int((n - t1) * 0.6) // (len2 * gpw) * (len2 * gpw)
    if tail_percent <= 0:
        t1 = t2 = n // wl * wl
    return t1, t2


def runs_of(n: int, L: int, tail1: int, tail2: int):
    """[(t0, t1)] of every run, in run order, as the kernel derives them from (run index, tail1, tail2)."""
    L2, L3 = (L >> 1 if L >= 2 else 1), (L >> 2 if L >= 4 else 1)
    R1 = tail1 // L
    R2 = R1 + (tail2 - tail1) // L2
    n_runs = R2 + (n - tail2 + L3 - 1) // L3
    out = []
    for run in range(n_runs):
        if run >= R2:
            Lr, t0 = L3, tail2 + (run - R2) * L3
        elif run >= R1:
            Lr, t0 = L2, tail1 + (run - R1) * L2
        else:
            Lr, t0 = L, run * L
        out.append((t0, min(t0 + Lr, n)))
    return out, R1, R2


def deal(n_runs: int, grid: int, gpw: int):
    """runs of every workgroup in the order its tickets hand them out: ticket k -> runs (k * grid + b) * gpw + {0..gpw-1}"""
    per = [[] for _ in range(grid)]
    for b in range(grid):
        k = 0
        while (k * grid + b) * gpw < n_runs:
            base = (k * grid + b) * gpw
            per[b].extend(r for r in range(base, min(base + gpw, n_runs)))
            k += 1
    return per


def run_launch(q0: np.ndarray, rows: np.ndarray, grads, grid: int, gpw: int, L: int, tail_percent: int, hot: np.ndarray,
               order: str = "round-robin", seed: int = 0):
    """One launch over triples whose item row is rows[t]: every triple adds grads(value it reads) to its row.  Hot
    rows (hot[row] True) take a workgroup's updates in its private delta and are read as q + own delta; at the end
    the deltas are summed into q.  The workgroups' runs are interleaved in time by `order`.  Returns (q, reads)."""
    n = len(rows)
    t1, t2 = zones(n, L, gpw, tail_percent)
    runs, _, _ = runs_of(n, L, t1, t2)
    per = deal(len(runs), grid, gpw)
    q = q0.astype(np.float64).copy()
    delta = np.zeros((grid, len(q)))
    reads = np.full(n, np.nan)
    cursor = [0] * grid
    rng = np.random.default_rng(seed)
    alive = [b for b in range(grid) if per[b]]
    while alive:
        b = alive[0] if order == "one-by-one" else (alive[int(rng.integers(len(alive)))] if order == "random" else alive[0])
        if order == "round-robin":
            alive.append(alive.pop(0))
            b = alive[-1]
        t0, t1_ = runs[per[b][cursor[b]]]
        for t in range(t0, t1_):
            r = rows[t]
            v = q[r] + (delta[b, r] if hot[r] else 0.0)
            reads[t] = v
            g = grads(v, t)
            if hot[r]:
                delta[b, r] += g
            else:
                q[r] += g
        cursor[b] += 1
        if cursor[b] == len(per[b]):
            alive.remove(b)
    q += delta.sum(0)  # the flush + the epilogue's fold
    return q, reads


def two_half_stream(n: int, L: int, tail_percent: int, K: int, users_half: int, seed: int, own_seen: int = 8,
                    neg_only: int = 2):
    """A launch's triples for ONE wave of two groups (G = 32, `gpw_active` = 2, grid 1) whose groups never share a
    row: wave-load k deals run 2k to group 0 and run 2k + 1 to group 1 (`deal` with grid 1, gpw 2), so the even runs
    take only half A — users 1..users_half, items 1..K — and the odd runs only half B — users users_half + 1 ..
    2 users_half, items K + 1 .. 2K.  Every user has seen ALL of the other half (and `own_seen` or fewer items of
    its own), so a sampler can only pick a negative from the user's own half; the given negatives are drawn there
    too.  Each half is a sequence of users with 1..12 consecutive triples (positives Zipf-skewed inside the half),
    laid into its runs in order: users are cut by run boundaries.  The last `neg_only` items of each half are never
    a positive (rows that only the negative's path reads and updates).  Run lengths and zones are those of `zones` /
    `runs_of` with gpw = 2.  Returns dict(users, pos, neg, indptr, indices, half_of_user, half_of_item, runs, I, U)."""
    rng = np.random.default_rng(seed)
    U, I = 2 * users_half + 1, 2 * K + 1
    half_u = np.full(U, -1)
    half_u[1:users_half + 1], half_u[users_half + 1:] = 0, 1
    half_i = np.full(I, -1)
    half_i[1:K + 1], half_i[K + 1:] = 0, 1
    items_of = [np.arange(1, K + 1, dtype=np.int32), np.arange(K + 1, 2 * K + 1, dtype=np.int32)]
    rows = [np.zeros(0, np.int32)]
    for u in range(1, U):
        h = half_u[u]
        own = rng.choice(items_of[h], size=int(rng.integers(0, own_seen + 1)), replace=False)
        rows.append(np.sort(np.concatenate([own, items_of[1 - h]])).astype(np.int32))
    indptr = np.zeros(U + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    t1, t2 = zones(n, L, 2, tail_percent)
    runs, _, _ = runs_of(n, L, t1, t2)
    need = [sum(b - a for r, (a, b) in enumerate(runs) if r % 2 == h) for h in (0, 1)]
    seqs = []
    for h in (0, 1):
        us = []
        while len(us) < need[h]:
            us += [int(rng.integers(1, users_half + 1)) + h * users_half] * int(rng.integers(1, 13))
        us = np.asarray(us[:need[h]], np.int32)
        pos = (items_of[h][0] + (rng.zipf(1.4, need[h]) - 1) % (K - neg_only)).astype(np.int32)
        neg = rng.choice(items_of[h], size=need[h]).astype(np.int32)
        seqs.append((us, pos, neg))
    users, pos, neg = (np.zeros(n, np.int32) for _ in range(3))
    at = [0, 0]
    for r, (a, b) in enumerate(runs):
        h, k = r % 2, at[r % 2]
        users[a:b], pos[a:b], neg[a:b] = (s[k:k + b - a] for s in seqs[h])
        at[h] += b - a
    return dict(users=users, pos=pos, neg=neg, indptr=indptr, indices=np.concatenate(rows), half_of_user=half_u,
                half_of_item=half_i, runs=runs, I=I, U=U)
