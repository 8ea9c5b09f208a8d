"""Top-K recommendation on the HIP engine: the k best unseen items of a list of users from one fused
kernel (`bpr_topk_rows`, csrc/bpr_topk.hip) — scores, exclusion of item 0 and of the user's seen
items, and the selection, with no [n, I] score matrix.  The reference ranks through full logits
(example.py:195-230; the preds.jsonl / user-metrics.jsonl savers of experiments/options.py:319-351).

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr._serving import best_items, query

TOPK_MAX = 128  # bpr_topk_rows: largest k


def workspace_bytes(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_topk_workspace`: bytes of device workspace a call of this shape needs."""
    return query("bpr_topk_workspace", n, num_items, d, k, item_slices, ctype=ctypes.c_int64)


def slices(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_topk_slices`: the slice count a call of this shape runs with."""
    return query("bpr_topk_slices", n, num_items, d, k, item_slices)


@torch.no_grad()
def recommend(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor,
              k: int, seen_indptr: Optional[torch.Tensor] = None,
              seen_indices: Optional[torch.Tensor] = None, *, item_slices: int = 0, check_users: bool = True,
              item_filter: Optional[torch.Tensor] = None):
    """The `k` best items of every user of `users` by <P[u], Q[i]> (+ item_bias[i]), item 0 and
    the user's row of the seen CSR (int64 [U+1], int32 sorted per row; None: only item 0) left out.

    Returns (items [n, k] int32, scores [n, k] float32): rows sorted by score descending, ties by
    ascending item id; a row with fewer than k eligible items ends in item -1 / score -inf.
    A NaN score (a NaN in a row, 0 * inf, inf - inf) is never returned, so such a row may end in
    padding although items are left; +inf and -inf scores are ordered like any other, and a real
    item scoring -inf keeps its id: only the padding is item -1 (tests/test_gpu_chain.py).  The
    result does not depend on n, on the order of `users` or on `item_slices` (0: the library
    chooses how many workgroups share the item range of a user tile).  Runs on the current stream.
    The kernel reads P[user] and the user's CSR row unchecked, so the ids are range-checked here
    first, which waits for the device; `check_users=False` leaves that out (ids known to be valid:
    a serving loop, a captured graph).

    `item_filter` (None: the whole catalogue): a packed filter of `revisit_bpr.item_filter.pack_item_filter` over
    the I items, on the tables' device; only items whose bit is set are eligible — the result is the unfiltered
    ranking restricted to them, bit for bit, cut to k (`bpr_topk_rows_filtered`).
    """
    return best_items("topk", "recommend", TOPK_MAX, P, Q, item_bias, users, k, seen_indptr, seen_indices,
                      item_slices=item_slices, check_users=check_users, item_filter=item_filter)
