"""Neighbour search on the HIP engine: the k rows of a table most similar to each of a list of query rows, by
cosine or by dot product, from one fused kernel (`bpr_neighbors_rows`, csrc/bpr_neighbors.hip) — scores, the
exclusions and the selection, with no [n, N] score matrix.  `similar_items` / `similar_users` are the usual pair of
an implicit-feedback library; `neighbors` is what they are made of.  The reference has no such call.

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr.item_filter import check_item_filter, check_item_filter_early
from revisit_bpr._serving import _table, call_rows, int32_ids, need_rocm, ptr, query, sliced_workspace
from revisit_bpr.recommend import TOPK_MAX

METRICS = {"dot": native.SIM_DOT, "cosine": native.SIM_COSINE}


def _metric(metric: str) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, not {metric!r}")
    return METRICS[metric]


def workspace_bytes(n: int, num_rows: int, d: int, k: int, metric: str = "cosine", item_slices: int = 0) -> int:
    """`bpr_neighbors_workspace`: bytes of device workspace a call of this shape needs."""
    return query("bpr_neighbors_workspace", n, num_rows, d, k, _metric(metric), item_slices, ctype=ctypes.c_int64)


def slices(n: int, num_rows: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_neighbors_slices`: the slice count a call of this shape runs with."""
    return query("bpr_neighbors_slices", n, num_rows, d, k, item_slices)


@torch.no_grad()
def neighbors(X: torch.Tensor, T: torch.Tensor, rows: torch.Tensor, k: int, *, metric: str = "cosine",
              exclude: Optional[torch.Tensor] = None, first: int = 0, item_slices: int = 0,
              check_rows: bool = True, item_filter: Optional[torch.Tensor] = None):
    """The `k` rows of `T` [N, d] most similar to each query `X[rows[r]]` (`X` [*, d]: `T` itself or another
    table of the same d), by `metric`: "cosine" (<x, t> / (|x| |t|)) or "dot" (<x, t>, the score of `recommend`
    without a bias).  Left out of row r: ids of `T` below `first`, the id `exclude[r]` (`exclude` None, or an
    entry below 0: none) and, under cosine, rows of `T` with a zero (or NaN) norm; a query with such a norm gets a
    fully padded row.

    Returns (ids [n, k] int32, scores [n, k] float32): rows sorted by score descending, ties by ascending id; a
    row with fewer than k eligible rows of `T` ends in id -1 / score -inf.
    A NaN score (a NaN in a row, 0 * inf, inf - inf) is never returned, so such a row may end in padding although
    rows of `T` are left; +inf and -inf scores are ordered like any other, and a real row scoring -inf keeps its id:
    only the padding is id -1.  Under cosine a row whose sum of squares overflows has the norm factor +0: it stays
    eligible, with scores +-0 or NaN (tests/test_gpu_chain.py).  The result does not depend on n, on
    the order of `rows` or on `item_slices` (0: the library chooses how many workgroups share the table for a
    query tile); include/bprcore.h defines its bits.  Runs on the current stream.  The kernel reads `X[rows[r]]`
    unchecked, so `rows` are range-checked against `X` (and `exclude` against `T`) here first, which waits for
    the device; `check_rows=False` leaves that out (ids known to be valid: a serving loop, a captured graph).

    `item_filter` (None: the whole table): a packed filter of `revisit_bpr.item_filter.pack_item_filter` over the N
    rows of `T`.  Only rows whose bit is set are returned; `first`, `exclude` and the cosine rule apply as before,
    and so does every score: the result is the unfiltered call's on the eligible rows of `T` alone, ids mapped back,
    k ids where filtering after the cut returns fewer (`bpr_neighbors_rows_filtered`).  With `first=0` row 0's bit
    counts like any other.

    Rows folded in after training (`fold_in_items`, `fold_in`) are looked at against the catalogue with
    `neighbors(Q_new, Q, torch.arange(m), k, first=1)`: row r of the result is what the new item r resembles."""
    k = int(k)
    if k > TOPK_MAX:
        raise ValueError(f"k = {k}: neighbors returns at most {TOPK_MAX} ids per query")
    if k < 1:
        raise ValueError("k must be at least 1")
    code = _metric(metric)
    first = int(first)
    if first < 0:
        raise ValueError("first must be at least 0")
    item_filter = check_item_filter_early(item_filter, T)
    need_rocm("neighbors", "the tables and the row list", (X, T, rows, exclude, item_filter),
              (X, T, rows, exclude, item_filter), "X")
    native.load()
    same = X is T
    T = _table(T, "T")
    X = T if same else _table(X, "X")
    if X.dim() != 2 or T.dim() != 2 or X.shape[1] != T.shape[1]:
        raise ValueError("X [*, d] and T [N, d] must share the embedding dim")
    (N, d), dev = T.shape, X.device
    item_filter = check_item_filter(item_filter, N)
    rows = int32_ids(rows, strict=False)
    n = rows.numel()
    if exclude is not None:
        exclude = int32_ids(exclude, strict=False)
        if exclude.numel() != n:
            raise ValueError("exclude must have one entry per query")
    if check_rows and n:
        if bool(((rows < 0) | (rows >= X.shape[0])).any()):
            raise ValueError("row id out of range")
        if exclude is not None and bool((exclude >= N).any()):
            raise ValueError("exclude id out of range")
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    item_slices, ws, ws_bytes = sliced_workspace("neighbors", (n, N, d, k), item_slices, dev, pre=(code,))
    call_rows("neighbors", dev,
              (X.data_ptr(), T.data_ptr(), N, d, rows.data_ptr(), n, ptr(exclude), first, code), item_filter,
              (k, item_slices, ptr(ws), ws_bytes, ids.data_ptr(), scores.data_ptr()))
    return ids, scores


def similar_items(Q: torch.Tensor, items: torch.Tensor, k: int, metric: str = "cosine", **kwargs):
    """The `k` items most similar to each item of `items` by their rows of the item table `Q`: `neighbors(Q, Q,
    items, k, exclude=items, first=1)` — never the item itself, never the padding item 0, never a NaN score
    (`neighbors` says what +-inf scores do).  A freshly folded-in
    item row is not in `Q`: `neighbors(Q_new, Q, torch.arange(m), k, first=1)`."""
    return neighbors(Q, Q, items, k, metric=metric, exclude=items, first=1, **kwargs)


def similar_users(P: torch.Tensor, users: torch.Tensor, k: int, metric: str = "cosine", **kwargs):
    """The `k` users most similar to each user of `users` by their rows of the user table `P`: `neighbors(P, P,
    users, k, exclude=users, first=0)` — never the user itself, never a NaN score (`neighbors` says what +-inf scores
    do); user 0 is a user like any other.  A freshly
    folded-in user row is not in `P`: `neighbors(P_new, P, torch.arange(m), k)`."""
    return neighbors(P, P, users, k, metric=metric, exclude=users, first=0, **kwargs)
