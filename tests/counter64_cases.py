"""Counters, seed and inputs shared by tests/test_counter64_cpu.py and tests/test_gpu_counter64.py.

Every negative is keyed by Philox4x32-10 with key = the 64-bit seed and counter = the 64-bit offset + position, split
by the kernels into a low and a high 32-bit word.  The offsets below put the high word, and the carry into it, inside a
launch; the seed has a non-zero high word and its top bit set (an unsigned 64-bit value through ctypes).

Everything here is numpy and the CPU oracle: the CPU module checks on these inputs that a stream drawn at a WRONG
counter (high word dropped, carry not propagated) differs from the right one almost everywhere, so that the GPU
module's comparisons with the oracle cannot pass by accident.  Oracle picks are computed once per (inputs, counter)
and shared (`uniform`, `adaptive`: cached, never written to).
"""
import numpy as np

import oracle

SEED = 0x9E3779B97F4A7C15
M32 = 0xFFFFFFFF
OFFSETS = ("carry", "rank1", "rank7_carry")


def wrap_default(n):
    """Positions before the low word wraps: n // 2 - 3 keeps the wrap off every run, group, wave and batch boundary."""
    return n // 2 - 3


def offset_of(name, n, wrap=None):
    """The counter of position 0.  `wrap`: how many positions come before the low word wraps (carry offsets)."""
    w = wrap_default(n) if wrap is None else wrap
    return {"carry": 2 ** 32 - w, "rank1": (1 << 40) + 12345, "rank7_carry": (7 << 40) + 2 ** 32 - w}[name]


def wrap_of(offset, n):
    """Positions of an n-triple call before the low word of its counter wraps (n: it does not)."""
    return min(n, 2 ** 32 - (offset & M32))


# ---- inputs of the GPU cases (the recipes of the low-offset tests they extend) ---------------------------------------
def rand_problem(*a, **kw):
    from test_gpu_parity import rand_problem as rp

    return rp(*a, **kw)


_problems = {}


def stream_problem(d, lds=False):
    """test_stream_picks_match_the_oracle_at_full_concurrency's problem (lds: its LDS-tier counterpart's, I = 700)."""
    key = ("stream", d, lds)
    if key not in _problems:
        U, I, n = 500, 700, 20_000
        P, Q, indptr, indices, users, pos, _ = rand_problem(U, I, d, 150, seed=40 + d + (I if lds else 0), B=n)
        P *= 6
        Q *= 6
        _problems[key] = dict(P=P, Q=Q, indptr=indptr, indices=indices, users=users, pos=pos, I=I, p=0.03)
    return _problems[key]


def seq_problem():
    """test_stream_sequential_limit_equals_b1_sgd's problem (d = 256: one triple per wave)."""
    if "seq" not in _problems:
        d, U, I, n = 256, 60, 90, 400
        P, Q, indptr, indices, users, pos, _ = rand_problem(U, I, d, 30, seed=5, B=n)
        P *= 8
        Q *= 8
        _problems["seq"] = dict(P=P, Q=Q, indptr=indptr, indices=indices, users=users, pos=pos, I=I, p=0.1)
    return _problems["seq"]


def synthetic_problem(d, n):
    """The problem of test_sequential_limit_with_on_device_sampling and test_train_strict_epoch_driver: 300 users,
    200 items, the first n triples of a permutation of the 6,000."""
    key = ("synthetic", d, n)
    if key not in _problems:
        from revisit_bpr.datasets import synthetic

        data = synthetic.generate(300, 200, 6000, median_per_user=12, seed=2)
        rng = np.random.default_rng(1)
        P = ((rng.random((data.num_users, d)) - 0.5) / d * 4).astype(np.float32)
        Q = ((rng.random((data.num_items, d)) - 0.5) / d * 4).astype(np.float32)
        P[0] = 0
        Q[0] = 0
        perm = rng.permutation(data.nnz)[:n]
        _problems[key] = dict(P=P, Q=Q, indptr=data.indptr, indices=data.indices, users=data.users[perm].copy(),
                              pos=data.items[perm].copy(), I=data.num_items, p=0.05)
    return _problems[key]


def vstream_full_problem():
    """test_full_concurrency_picks_match_the_oracle's problem (tests/test_gpu_vstream.py), unshuffled."""
    if "vfull" not in _problems:
        from revisit_bpr.datasets import synthetic

        data = synthetic.generate(2000, 700, 60_000, median_per_user=20, seed=3)
        d = 128
        rng = np.random.default_rng(2)
        P = ((rng.random((data.num_users, d)) - 0.5) / d * 4).astype(np.float32)
        Q = ((rng.random((data.num_items, d)) - 0.5) / d * 4).astype(np.float32)
        P[0] = 0
        Q[0] = 0
        _problems["vfull"] = dict(P=P, Q=Q, indptr=data.indptr, indices=data.indices, users=data.users,
                                  pos=data.items, I=data.num_items, p=0.02)
    return _problems["vfull"]


# The fold-in modules' fixtures hold users who have seen every item, or all but one: their negative does not depend
# on the counter at all, and with 50 items two independent draws of the others collide too often for the power check
# (at least 90 % of the positions differ).  The cases below are the modules' recipes (`make_rows`, `tables`) on 300
# items without the saturated rows.
FOLD_I, FOLD_LENGTHS, FOLD_EPOCHS = 300, [0, 1, 2, 3, 9, 17, 40, 120], 3
FOLD_ADAPTIVE_EPOCHS, FOLD_P_GEO = 8, 0.2


def _rows(lengths, n_ids, rng, first):
    rows = [np.sort(rng.choice(np.arange(first, n_ids), size=k, replace=False)).astype(np.int32) for k in lengths]
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), np.concatenate(rows).astype(np.int32)


def foldin_problem(d):
    """New users (rows of a CSR over the items) for `fold_in`: the triple at CSR position k belongs to row users_of[k]."""
    key = ("foldin", d)
    if key not in _problems:
        rng = np.random.default_rng(100 + d)
        Q = rng.normal(0, 0.5, (FOLD_I, d)).astype(np.float32)
        Q[0] = 0
        b = rng.normal(0, 0.5, FOLD_I).astype(np.float32)
        P0 = rng.normal(0, 0.1, (len(FOLD_LENGTHS), d)).astype(np.float32)
        indptr, items = _rows(FOLD_LENGTHS, FOLD_I, np.random.default_rng(7), 1)
        users_of = np.repeat(np.arange(len(FOLD_LENGTHS)), FOLD_LENGTHS).astype(np.int32)
        _problems[key] = dict(P=P0, Q=Q, b=b, indptr=indptr, indices=items, users_of=users_of, I=FOLD_I, p=FOLD_P_GEO,
                              nnz=int(indptr[-1]))
    return _problems[key]


FOLD_ITEMS_U, FOLD_ITEMS_LENGTHS = 40, [0, 1, 2, 3, 9, 17, 33, 40]
FOLD_ITEMS_SEEN = [0, 1, 17, 48, 49] + [3, 7, 11, 5, 9] * 7


def foldin_items_problem(d):
    """New items (rows of a CSR over the users) for `fold_in_items`: the triple at CSR position k is user users[k]'s,
    and its negative is an item of the I = 300 that user has not seen."""
    key = ("foldin_items", d)
    if key not in _problems:
        rng = np.random.default_rng(100 + d)
        m = len(FOLD_ITEMS_LENGTHS)
        P = rng.normal(0, 0.5, (FOLD_ITEMS_U, d)).astype(np.float32)
        Q = rng.normal(0, 0.5, (FOLD_I, d)).astype(np.float32)
        Q[0] = 0
        b = rng.normal(0, 0.5, FOLD_I).astype(np.float32)
        Q0, b0 = rng.normal(0, 0.1, (m, d)).astype(np.float32), rng.normal(0, 0.1, m).astype(np.float32)
        r7 = np.random.default_rng(7)
        indptr, users = _rows(FOLD_ITEMS_LENGTHS, FOLD_ITEMS_U, r7, 0)
        seen_indptr, seen_indices = _rows(FOLD_ITEMS_SEEN, FOLD_I, r7, 1)
        _problems[key] = dict(P=P, Q=Q, b=b, Q0=Q0, b0=b0, indptr=indptr, users=users, seen_indptr=seen_indptr,
                              seen_indices=seen_indices, I=FOLD_I, nnz=int(indptr[-1]))
    return _problems[key]


# ---- the oracle's picks, once per (inputs, counter) --------------------------------------------------------------------
_snapshots, _picks = {}, {}


def snapshot(pr):
    """(sigma, order) of the oracle for the problem's item table."""
    if id(pr) not in _snapshots:
        QT, sigma = oracle.adaptive_stats(pr["Q"])
        _snapshots[id(pr)] = (pr, sigma, oracle.adaptive_order(QT))
    return _snapshots[id(pr)][1:]


def _frozen(a):
    a.setflags(write=False)
    return a


def uniform(pr, users, offset, tag=None, indptr=None, indices=None):
    """oracle.sample_uniform for `users` at `offset`; tag: cache key of a user list used by several tests."""
    key = None if tag is None else ("u", id(pr), tag, offset)
    if key in _picks:
        assert np.array_equal(_picks[key][0], users)
        return _picks[key][1]
    ip = (pr["seen_indptr"] if "seen_indptr" in pr else pr["indptr"]) if indptr is None else indptr
    ix = (pr["seen_indices"] if "seen_indices" in pr else pr["indices"]) if indices is None else indices
    out = _frozen(oracle.sample_uniform(ip, ix, pr["I"], np.ascontiguousarray(users, np.int32), SEED, offset))
    if key is not None:
        _picks[key] = (np.array(users), out)
    return out


def adaptive(pr, users, offset, tag=None):
    """oracle.sample_adaptive (negatives, factors, ranks) for `users` at `offset` on the problem's frozen tables."""
    key = None if tag is None else ("a", id(pr), tag, offset)
    if key in _picks:
        assert np.array_equal(_picks[key][0], users)
        return _picks[key][1]
    sigma, order = snapshot(pr)
    out = tuple(_frozen(x) for x in oracle.sample_adaptive(pr["P"], sigma, order, pr["indptr"], pr["indices"],
                                                           np.ascontiguousarray(users, np.int32), pr["p"], SEED, offset))
    if key is not None:
        _picks[key] = (np.array(users), out)
    return out


# ---- what a kernel with a broken counter would draw ------------------------------------------------------------------
def wrong_streams(draw, users, offset):
    """`draw(users, offset)` -> picks.  Returns {name: (picks of the broken counter, positions that count)}:
      high_dropped  counter = (offset + t) & 0xFFFFFFFF, every position (where the high word is zero to begin with:
                    the positions after the wrap);
      no_carry      counter = (offset & ~0xFFFFFFFF) | ((offset + t) & 0xFFFFFFFF): the low word wraps and the high word
                    stays, the positions after the wrap (offsets whose low word wraps inside the call only)."""
    n = len(users)
    w = wrap_of(offset, n)
    hi = offset & ~M32
    out = {}
    dropped = np.concatenate([draw(users[:w], offset & M32), draw(users[w:], 0)]) if w < n else draw(users, offset & M32)
    out["high_dropped"] = (dropped, slice(0, n) if hi else slice(w, n))
    if w < n:  # (high word zero: the same broken stream as high_dropped)
        out["no_carry"] = (np.concatenate([draw(users[:w], offset), draw(users[w:], hi)]), slice(w, n))
    return {k: v for k, v in out.items() if v[1].stop > v[1].start}
