"""Inputs for the ROC-AUC tests (tests/test_auc_model_cpu.py, tests/test_gpu_auc.py) — TEST INFRASTRUCTURE ONLY.
numpy only; everything comes from fixed seeds.  Three families:

  small_rows()        I <= 64, every T from 1 to I: the rows on which the model (tests/auc_model.py) is pinned
  boundary_rows(cls)  the rows at the kernel's own constants (256 threads, 4,096 positives in LDS), by score class
  family()            one small adversarial evaluation dataset for evaluate_topk / evaluate_ranked

Every GPU row keeps T * (I - T) <= 2^24 = TN_MAX: values lie in [0, 1], where float32 is spaced at most 2^-24 apart,
and one pair moves the quotient by 1 / (T (I - T)) >= 2^-24, so a single miscounted pair changes the float32 bits
(tests/test_auc_model_cpu.py::test_one_pair_changes_the_float32_up_to_2_pow_24 checks the claim itself)."""
import functools

import numpy as np

from auc_model import auc_rows

TN_MAX = 1 << 24
MASKED = np.float32(-1e13)
CLASSES = "abcde"
TS = (1, 2, 255, 256, 257, 1023, 4095, 4096)
GAPS = (1, 255, 256, 257)  # I - T
TINY = np.array([np.inf, -np.inf, 0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127, -(2.0 ** -127), 2.0 ** -126],
                np.float32)


def scores_of(cls, rng, I, pos=None):
    """One row of a score class.  a: distinct normals; b: multiples of 1 / 2 in [-3, 3]; c: all equal; d: (b) with
    5 % of the entries, column 0 and a positive at -1e13; e: (b) with +-inf, +-0 and subnormals mixed in."""
    if cls == "a":
        return ((rng.permutation(I) - I // 2) * 0.25 + 0.125).astype(np.float32)  # (exact, never 0)
    if cls == "c":
        return np.full(I, 0.75, np.float32)
    s = (rng.integers(-6, 7, I) / 2).astype(np.float32)
    if cls == "d":
        s[rng.random(I) < 0.05] = MASKED
        s[0] = MASKED
        if pos is not None and len(pos) >= 2:
            s[pos[0]] = MASKED
    if cls == "e":
        at = rng.random(I) < 0.3
        s[at] = rng.choice(TINY, int(at.sum()))
    return s


class Rows:
    """Rows of ONE width I: scores [n, I], the targets as a CSR in random order (ptr, items) and ascending
    (items_sorted), and the model's answer (wins, T, n_neg, value)."""

    def __init__(self, scores, targets):
        self.scores = np.ascontiguousarray(scores, np.float32)
        self.n, self.I = self.scores.shape
        self.ptr = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int64)
        self.items = np.concatenate(list(targets) + [np.zeros(0, np.int32)]).astype(np.int32)
        self.items_sorted = np.concatenate([np.sort(t) for t in targets] + [np.zeros(0, np.int32)]).astype(np.int32)
        self.wins, self.T, self.n_neg, self.value = auc_rows(self.scores, self.ptr, self.items)

    def take(self, order):
        """The rows `order`, as a new CSR (the model's answers are taken along, not recomputed)."""
        r = Rows.__new__(Rows)
        order = np.asarray(order)
        r.scores = np.ascontiguousarray(self.scores[order])
        r.n, r.I = len(order), self.I
        tg = [self.items[self.ptr[i]:self.ptr[i + 1]] for i in order]
        r.ptr = np.concatenate([[0], np.cumsum([len(t) for t in tg])]).astype(np.int64)
        r.items = np.concatenate(tg + [np.zeros(0, np.int32)]).astype(np.int32)
        r.items_sorted = np.concatenate([np.sort(t) for t in tg] + [np.zeros(0, np.int32)]).astype(np.int32)
        r.wins, r.T, r.n_neg, r.value = self.wins[order], self.T[order], self.n_neg[order], self.value[order]
        return r


def draw(rng, I, T):
    return rng.choice(I, size=T, replace=False).astype(np.int32)  # (random order; id 0 is an id like any other)


def rows_of(cls, rng, I, Ts):
    targets = [draw(rng, I, T) for T in Ts]
    return Rows(np.stack([scores_of(cls, rng, I, t) for t in targets]), targets)


def boundary_shapes():
    """(T, I) of section 1: T at 1, 2, around the 256 threads and at the 4,096 LDS slots; I - T at 1 and around 256;
    for the two largest T also I - T = 4,096 (T (I - T) = 2^24 exactly at T = 4,096); I = 2; I = 200 < 256 threads."""
    shapes = [(T, T + g) for T in TS for g in GAPS] + [(4095, 4095 + 4096), (4096, 4096 + 4096), (1, 2), (7, 200)]
    return sorted(set(shapes), key=lambda ti: (ti[1], ti[0]))


@functools.lru_cache(maxsize=None)
def boundary_rows(cls):
    """The rows of boundary_shapes() in score class `cls`, grouped by width (a launch has one I): a list of Rows.
    Rows of different T share a launch wherever the shapes share an I (I = 257: T = 1, 2 and 256; I = 512: T = 255,
    256 and 257; ...)."""
    rng = np.random.default_rng(100 + CLASSES.index(cls))
    by_I = {}
    for T, I in boundary_shapes():
        by_I.setdefault(I, []).append(T)
    return [rows_of(cls, rng, I, Ts) for I, Ts in by_I.items()]


MIXED_I = 8192


@functools.lru_cache(maxsize=None)
def mixed_rows(cls):
    """40 rows of ONE launch, I = 8,192 (every T up to 4,096 keeps T (I - T) <= 2^24 there): the eight boundary T and
    32 small random ones."""
    rng = np.random.default_rng(200 + CLASSES.index(cls))
    Ts = list(TS) + [int(t) for t in rng.integers(1, 300, 32)]
    order = rng.permutation(len(Ts))
    return rows_of(cls, rng, MIXED_I, [Ts[i] for i in order])


def small_rows(seed=5):
    """[(scores [I] float32, target ids)]: I in 1 .. 64 and every T from 1 to I (T = I: no negatives); tie-heavy
    scores (multiples of 1 / 2) with masked entries, +-inf, +-0 and subnormals mixed in."""
    rng = np.random.default_rng(seed)
    out = []
    for I in (1, 2, 3, 7, 31, 64):
        for T in range(1, I + 1):
            s = (rng.integers(-4, 5, I) / 2).astype(np.float32)
            kind = T % 3
            if kind == 1:
                s[rng.random(I) < 0.2] = MASKED
                s[0] = MASKED
            elif kind == 2:
                at = rng.random(I) < 0.5
                s[at] = rng.choice(TINY, int(at.sum()))
            out.append((s, draw(rng, I, T)))
    return out


def nan_rows(rows, seed=9):
    """The rows of small_rows() with I >= 3 again, with NaN among the positives (kind 0), the negatives (1), both (2)
    or everywhere (3)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (s, t) in enumerate(rows):
        if len(s) < 3:
            continue
        s, kind = s.copy(), k % 4
        is_pos = np.zeros(len(s), bool)
        is_pos[t] = True
        hit = rng.random(len(s)) < 0.3
        if kind == 0:
            s[hit & is_pos] = np.nan
            s[t[0]] = np.nan
        elif kind == 1:
            s[hit & ~is_pos] = np.nan
            s[np.flatnonzero(~is_pos)[:1]] = np.nan  # (none where T = I)
        elif kind == 2:
            s[hit] = np.nan
            s[t[0]] = np.nan
        else:
            s[:] = np.nan
        out.append((s, t))
    return out


class Family:
    pass


@functools.lru_cache(maxsize=None)
def family():
    """U = 24 users, I = 4,200 items, d = 8; tables from {-4 .. 4} / 4 and a bias from multiples of 1 / 4 (every score
    a multiple of 1 / 16, exact in fp32 in any order: the CPU and GPU GEMMs agree bit for bit, ties are plentiful).
    Seen CSR: user 1 has seen nothing, user 2 all but 40 items.  The eval CSR starts two rows into a longer one
    (`eval_indptr` does not start at 0) and holds, in this order: no target, one target, a duplicate, a target listed
    three times, a seen target, target id 0, 4,096 targets, 4,097 targets (the sort-based form inside evaluate_topk),
    and four ordinary rows.  `logits` [E, I] are the eval loop's scores (seen items and item 0 at -1e13) and `model`
    the answer of tests/auc_model.py for them (t_max=None: evaluate_topk computes every row)."""
    f = Family()
    U, I, d = 24, 4200, 8
    rng = np.random.default_rng(4200)
    P = (rng.integers(-4, 5, (U, d)) / 4).astype(np.float32)
    Q = (rng.integers(-4, 5, (I, d)) / 4).astype(np.float32)
    b = (rng.integers(-8, 9, I) / 4).astype(np.float32)
    S = P.astype(np.float64) @ Q.T.astype(np.float64) + b.astype(np.float64)
    assert np.array_equal(S, S.astype(np.float32))
    seen = []
    for u in range(U):
        if u == 1:
            seen.append(np.zeros(0, np.int32))
        elif u == 2:
            seen.append(np.setdiff1d(np.arange(1, I), rng.choice(np.arange(1, I), 40, replace=False)).astype(np.int32))
        else:
            seen.append(np.flatnonzero(rng.random(I - 1) < 0.2).astype(np.int32) + 1)
    f.seen_indptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])]).astype(np.int64)
    f.seen_indices = np.concatenate(seen).astype(np.int32)

    def unseen(u, k):
        return rng.choice(np.setdiff1d(np.arange(1, I), seen[u]), k, replace=False).astype(np.int32)

    users = np.array([5, 1, 7, 8, 9, 10, 3, 4, 2, 11, 1, 12], np.int32)
    tg = [np.zeros(0, np.int32), unseen(1, 1)]
    x = unseen(7, 3)
    tg.append(np.array([x[0], x[1], x[0], x[2]], np.int32))              # a duplicate
    x = unseen(8, 2)
    tg.append(np.array([x[0], x[1], x[0], x[0]], np.int32))              # one target three times
    tg.append(np.append(unseen(9, 2), seen[9][3]).astype(np.int32))      # a seen target
    tg.append(np.append(unseen(10, 2), 0).astype(np.int32))              # target id 0
    tg.append(rng.choice(np.arange(1, I), 4096, replace=False).astype(np.int32))
    tg.append(rng.choice(np.arange(1, I), 4097, replace=False).astype(np.int32))
    tg.append(unseen(2, 5))                                              # (of the user who has seen nearly everything)
    tg += [unseen(11, 30), unseen(1, 300), unseen(12, 2)]
    f.NO_TARGET, f.DUPLICATES, f.KERNEL_MAX, f.SORTED_FORM = 0, (2, 3), 6, 7
    lead = [np.array([3, 9], np.int32), np.array([4], np.int32)]         # two rows in front of the slice in use
    f.lead = len(lead)
    all_rows = lead + tg
    f.full_indptr = np.concatenate([[0], np.cumsum([len(t) for t in all_rows])]).astype(np.int64)
    f.eval_indptr = f.full_indptr[f.lead:]
    f.eval_items = np.concatenate(all_rows).astype(np.int32)
    assert f.eval_indptr[0] > 0
    f.P, f.Q, f.b, f.users, f.I, f.E = P, Q, b, users, I, len(users)
    logits = S[users].astype(np.float32)
    for e, u in enumerate(users):
        logits[e, seen[u]] = MASKED
    logits[:, 0] = MASKED
    f.logits = logits
    f.model = auc_rows(logits, f.eval_indptr, f.eval_items, t_max=None)
    wins, T, n_neg, _ = f.model
    assert T[f.NO_TARGET] == 0 and T[1] == 1 and T[2] == 3 and T[3] == 2 and T[6] == 4096 and T[7] == 4097
    assert (T * n_neg).max() <= TN_MAX
    assert len(np.unique(logits[6][1:50])) < 49  # ties are plentiful
    return f


def one_user(f, e, device):
    """evaluate_topk(auc=True) on the one-user slice e of family() on `device`: its `auc` is that row's float32."""
    import torch

    from revisit_bpr.evaluation import evaluate_topk

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
    out = evaluate_topk(t(f.P), t(f.Q), t(f.b), t(f.users[e:e + 1]), t(f.full_indptr)[f.lead + e:f.lead + e + 2],
                        t(f.eval_items), t(f.seen_indptr), t(f.seen_indices), ks=(5,), auc=True)
    return np.float32(out["auc"])


def whole_call(f, rows, device, block=7):
    """... on the users rows[0] .. rows[1] - 1 in blocks of `block`: the mean."""
    import torch

    from revisit_bpr.evaluation import evaluate_topk

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
    lo, hi = rows
    return evaluate_topk(t(f.P), t(f.Q), t(f.b), t(f.users[lo:hi]), t(f.full_indptr)[f.lead + lo:f.lead + hi + 1],
                         t(f.eval_items), t(f.seen_indptr), t(f.seen_indices), ks=(5,), auc=True, block=block)["auc"]
