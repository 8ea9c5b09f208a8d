"""A numpy model of k_retrieve's selection for ONE row (revisit-bpr_amd/csrc/bpr_retrieve.hip): a threshold tau, a
need-count per item tile, compaction when count + need > cap, appends in arbitrary order, seen membership tested at
compaction for what was appended since the last one.  It models the selection only: scores are given.

The order is the result's: score descending, ties by ascending id; a NaN score never enters."""
import numpy as np

TI = 128  # items of a tile (bpr_topk_plan.h)
NEG_INF = np.float32(-np.inf)
INT_MAX = 2 ** 31 - 1


def cap_of(k):
    """bpr_retrieve_plan.h, retrieve_cap: a power of two >= max(k + TI, 2 k)"""
    cap = 1
    while cap < max(k + TI, 2 * k):
        cap *= 2
    return cap


def better(s, i, ts, ti):
    return s > ts or (s == ts and i < ti)


def brute_force(scores, k, seen=()):
    """(ids, scores) of the k best eligible items: item 0, seen items and NaN scores left out; padded (-1, -inf)."""
    scores = np.asarray(scores, np.float32)
    ok = ~np.isnan(scores)
    ok[0] = False
    ok[np.asarray(list(seen), np.int64)] = False
    ids = np.flatnonzero(ok)
    top = ids[np.lexsort((ids, -scores[ids].astype(np.float64)))][:k]
    out_i = np.full(k, -1, np.int32)
    out_s = np.full(k, NEG_INF, np.float32)
    out_i[:len(top)] = top
    out_s[:len(top)] = scores[top]
    return out_i, out_s


class Row:
    """The state of one row and the three steps of a tile."""

    def __init__(self, k, cap=None, seen=()):
        self.k, self.cap = k, cap_of(k) if cap is None else cap
        assert self.cap >= k + TI
        self.seen = set(int(x) for x in seen)
        self.buf = []  # (score, id): at most cap
        self.checked = 0  # entries at the front known to be unseen
        self.tau = (NEG_INF, INT_MAX)  # everything beats it
        self.compactions = 0
        self.high_water = 0

    def compact(self):
        head, tail = self.buf[:self.checked], self.buf[self.checked:]
        left = head + [e for e in tail if e[1] not in self.seen]
        left.sort(key=lambda e: (-float(e[0]), e[1]))
        if len(left) >= self.k:
            self.tau = left[self.k - 1]
        self.buf = left[:self.k]
        self.checked = len(self.buf)
        self.compactions += 1
        return left

    def tile(self, ids, scores, rng=None):
        """ids / scores of one item tile (<= TI); rng: the order the appends take their slots in"""
        assert len(ids) <= TI
        beat = [(np.float32(s), int(i)) for i, s in zip(ids, scores) if i > 0 and better(s, i, *self.tau)]  # (A)
        if len(self.buf) + len(beat) > self.cap:  # (B)
            self.compact()
        app = [e for e in beat if better(e[0], e[1], *self.tau)]  # (C)
        if rng is not None:
            app = [app[j] for j in rng.permutation(len(app))]
        for e in app:
            assert len(self.buf) < self.cap  # the store guard never has to act
            self.buf.append(e)
        self.high_water = max(self.high_water, len(self.buf))

    def result(self):
        left = self.compact()[:self.k]
        out_i = np.full(self.k, -1, np.int32)
        out_s = np.full(self.k, NEG_INF, np.float32)
        for j, (s, i) in enumerate(left):
            out_i[j], out_s[j] = i, s
        return out_i, out_s


def retrieve_row(scores, k, seen=(), cap=None, rng=None, lo=0, hi=None):
    """The model over the items lo .. hi of `scores` ([I] float32, index = item id), tile by tile."""
    scores = np.asarray(scores, np.float32)
    hi = len(scores) if hi is None else hi
    row = Row(k, cap, seen)
    for t in range(lo // TI, -(-hi // TI)):
        ids = np.arange(max(t * TI, lo), min((t + 1) * TI, hi))
        row.tile(ids, scores[ids], rng)
    return row.result() + (row,)
