"""numpy model of the ROC-AUC contract of `bpr_auc_rows` (revisit-bpr_amd/csrc/bpr_eval.hip, include/bprcore.h) and of
the `auc` of `evaluation.evaluate_topk` / `evaluate_ranked` — TEST INFRASTRUCTURE ONLY.  An all-pairs count with
integer results; no torch, none of the product's metric classes, not the library.

For one row with scores s[0 .. I) (float32) and the SET Pos of its target ids (a listed id counts once):
    wins = #{(p, n) : p in Pos, n not in Pos, s[p] > s[n]}     IEEE '>': false when either side is NaN, -0 == +0,
                                                               subnormals by value, +-inf ordinary values
    T = |Pos|, n_neg = I - T
    value = float32(float64(wins) / (float64(T) * float64(n_neg)));  NaN when T == 0 or T == I (0 / 0), and when
            T > T_MAX = 4096, which the kernel leaves to its caller ("not computed"; `t_max=None`: no such limit)

Pinned against oracle/metrics_np.py and the product's dense RocAucMany by tests/test_auc_model_cpu.py, so that the GPU
tests (tests/test_gpu_auc.py) have a yardstick that does not come from the code under test."""
import numpy as np

T_MAX = 4096
CHUNK = 512  # positives compared at once: a [CHUNK, n_neg] bool block


def value_of(wins, T, n_neg):
    """The float32 the contract assigns to the integer counts."""
    if T == 0 or n_neg == 0:
        return np.float32(np.nan)
    return np.float32(np.float64(wins) / (np.float64(T) * np.float64(n_neg)))


def auc_row(scores_f32, target_ids, t_max=T_MAX):
    """-> (wins: int, T: int, n_neg: int, value: np.float32).  The counts are returned for every row, also where the
    value is NaN."""
    s = np.asarray(scores_f32)
    assert s.dtype == np.float32 and s.ndim == 1
    I = s.shape[0]
    ids = np.unique(np.asarray(target_ids, np.int64))  # the set
    assert ids.size == 0 or (ids[0] >= 0 and ids[-1] < I), "target ids lie in [0, I)"
    is_pos = np.zeros(I, bool)
    is_pos[ids] = True
    pos, neg = s[is_pos], s[~is_pos]
    T, n_neg = int(pos.size), int(neg.size)
    wins = 0
    with np.errstate(invalid="ignore"):
        for lo in range(0, T, CHUNK):
            wins += int((pos[lo:lo + CHUNK, None] > neg[None, :]).sum())
    if t_max is not None and T > t_max:
        return wins, T, n_neg, np.float32(np.nan)
    return wins, T, n_neg, value_of(wins, T, n_neg)


def auc_rows(scores_f32, indptr, items, t_max=T_MAX):
    """Rows of a CSR: row r of scores_f32 [n, I] with the targets items[indptr[r] : indptr[r + 1]] (indptr need not
    start at 0).  -> (wins int64 [n], T int64 [n], n_neg int64 [n], value float32 [n])."""
    S = np.asarray(scores_f32)
    n = S.shape[0]
    assert len(indptr) == n + 1
    out = [auc_row(S[r], items[indptr[r]:indptr[r + 1]], t_max) for r in range(n)]
    wins, T, n_neg = (np.array([o[k] for o in out], np.int64) for k in range(3))
    return wins, T, n_neg, np.array([o[3] for o in out], np.float32)


def bits(x):
    """float32 -> int32 patterns, every NaN as one: what "bit for bit" compares."""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    b = x.view(np.int32).copy()
    b[np.isnan(x)] = 0x7FC00000
    return b
