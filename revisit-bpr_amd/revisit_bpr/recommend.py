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

from revisit_bpr import native

TOPK_MAX = 128  # bpr_topk_rows: largest k


def workspace_bytes(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_topk_workspace`: bytes of device workspace a call of this shape needs."""
    out = ctypes.c_int64()
    native.check(native.load().bpr_topk_workspace(n, num_items, d, k, item_slices, ctypes.byref(out)))
    return int(out.value)


def slices(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_topk_slices`: the slice count a call of this shape runs with."""
    out = ctypes.c_int32()
    native.check(native.load().bpr_topk_slices(n, num_items, d, k, item_slices, ctypes.byref(out)))
    return int(out.value)


def _table(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    return t.detach().contiguous()


@torch.no_grad()
def recommend(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor,
              k: int, seen_indptr: Optional[torch.Tensor] = None,
              seen_indices: Optional[torch.Tensor] = None, *, item_slices: int = 0, check_users: bool = True):
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
    """
    k = int(k)
    if k > TOPK_MAX:
        raise ValueError(f"k = {k}: recommend returns at most {TOPK_MAX} items per user")
    if k < 1:
        raise ValueError("k must be at least 1")
    if not (P.is_cuda and Q.is_cuda and users.is_cuda and (item_bias is None or item_bias.is_cuda)):
        raise RuntimeError("recommend needs the tables and the user list on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != P.device for t in (Q, item_bias, users, seen_indptr, seen_indices)):
        raise RuntimeError("recommend needs every tensor on the device of P")
    lib = native.load()
    P, Q, item_bias = _table(P, "P"), _table(Q, "Q"), _table(item_bias, "item_bias")
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError("P [U, d] and Q [I, d] must share the embedding dim")
    (U, d), I = P.shape, Q.shape[0]
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    dev = P.device
    users = users.reshape(-1)
    if users.dtype != torch.int32:
        users = users.to(torch.int32)
    users = users.contiguous()
    n = users.numel()
    if (seen_indptr is None) != (seen_indices is None):
        raise ValueError("seen_indptr and seen_indices go together")
    if seen_indptr is not None:
        if seen_indptr.dtype != torch.int64 or seen_indices.dtype != torch.int32:
            raise ValueError("seen_indptr must be int64 and seen_indices int32")
        if seen_indptr.numel() != U + 1:
            raise ValueError("seen_indptr must have U+1 entries")
        seen_indptr, seen_indices = seen_indptr.contiguous(), seen_indices.contiguous()
    if check_users and n and bool(((users < 0) | (users >= U)).any()):
        raise ValueError("user id out of range")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    item_slices = slices(n, I, d, k, item_slices)  # the count this call runs with: the workspace is its own need
    ws_bytes = workspace_bytes(n, I, d, k, item_slices)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        native.check(lib.bpr_topk_rows(
            P.data_ptr(), Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d,
            users.data_ptr(), n, None if seen_indptr is None else seen_indptr.data_ptr(),
            None if seen_indices is None else seen_indices.data_ptr(), k, item_slices,
            None if ws is None else ws.data_ptr(), ws_bytes, items.data_ptr(), scores.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream))
    return items, scores
