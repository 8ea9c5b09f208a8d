"""Exact ranks of held-out items on the HIP engine: where each target of a user stands among the
user's unseen items, from one fused pass over the item table (`bpr_rank_rows`, csrc/bpr_rank.hip) —
scores, exclusion of item 0 and of the seen items, and the counting, with no [n, I] score matrix and
no cutoff.  The reference ranks through full logits (example.py:195-230; experiments/bpr/exp.py:369-374).

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr.item_filter import check_item_filter, check_item_filter_early
from revisit_bpr._serving import call_rows, int32_ids, need_rocm, ptr, query, seen_csr, sliced_workspace, tables

RANK_TMAX = 112  # bpr_rank_rows: targets of one kernel row (csrc/bpr_rank_plan.h); longer rows are split here


def workspace_bytes(n: int, num_items: int, d: int, item_slices: int = 0) -> int:
    """`bpr_rank_workspace`: bytes of device workspace a call of this shape needs."""
    return query("bpr_rank_workspace", n, num_items, d, item_slices, ctype=ctypes.c_int64)


def slices(n: int, num_items: int, d: int, item_slices: int = 0) -> int:
    """`bpr_rank_slices`: the slice count a call of this shape runs with."""
    return query("bpr_rank_slices", n, num_items, d, item_slices)


def split_rows(users: torch.Tensor, tgt_indptr: torch.Tensor, tmax: int = RANK_TMAX):
    """Rows of at most `tmax` targets: a longer row becomes ceil(len / tmax) consecutive rows of the
    same user over the same stretch of the target list (which is not touched, so the outputs stay
    aligned with it).  Returns (users, tgt_indptr) of the kernel rows."""
    lens = tgt_indptr[1:] - tgt_indptr[:-1]
    pieces = ((lens + (tmax - 1)) // tmax).clamp(min=1)
    first = torch.cumsum(pieces, 0) - pieces  # kernel row of a row's first piece
    total = int(pieces.sum())
    row = torch.repeat_interleave(torch.arange(lens.numel(), device=lens.device), pieces)
    k = torch.arange(total, device=lens.device) - first[row]
    starts = tgt_indptr[:-1][row] + k * tmax
    return users[row].contiguous(), torch.cat([starts, tgt_indptr[-1:]]).contiguous()


@torch.no_grad()
def rank_items(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor,
               tgt_indptr: torch.Tensor, tgt_items: torch.Tensor, seen_indptr: Optional[torch.Tensor] = None,
               seen_indices: Optional[torch.Tensor] = None, *, item_slices: int = 0, check_users: bool = True,
               item_filter: Optional[torch.Tensor] = None):
    """For every target of every row — row r is user `users[r]` with the targets
    `tgt_items[tgt_indptr[r]:tgt_indptr[r + 1]]` (int64 [n+1] starting at 0, int32; a user may appear
    in several rows) — its place among the user's ELIGIBLE items: items 1 .. I-1 that are not in the
    user's row of the seen CSR (int64 [U+1], int32 sorted per row; None: only item 0 is left out),
    `recommend`'s rule, scored by <P[u], Q[j]> (+ item_bias[j]) with `recommend`'s bits.

    Returns (rank, not_below, score), each aligned with `tgt_items`: rank (int32) = eligible items
    other than the target that come before it in `recommend`'s order (higher score, or equal score
    and lower id); not_below (int32) = eligible items other than the target that score at least as
    high; score (float32).  A target that is itself not eligible (id 0, out of range, or seen) has
    rank = not_below = -1 and score -inf.  Other targets of the user count as ordinary items, so the
    answer does not depend on how targets are grouped into rows, on the order of the rows or on
    `item_slices` (0: the library chooses); rows longer than RANK_TMAX are split here, invisibly.
    Runs on the current stream and waits for it (row lengths are read back; `bpr_rank_rows` reads
    them again for its own bound).  The kernel reads P[user] and the user's CSR row unchecked, so the
    ids are range-checked here first; `check_users=False` leaves that out.

    `item_filter` (None: the whole catalogue): a packed filter of `revisit_bpr.item_filter.pack_item_filter` over
    the I items.  An item is then eligible only if its bit is set as well, and a target whose bit is clear is itself
    not eligible (-1 / -1 / -inf).  Scores are untouched: the answer is the unfiltered call's on the catalogue
    compacted to item 0 and the filter's items in ascending order (`bpr_rank_rows_filtered`).  A segment's ranks
    cannot be had by cutting the unfiltered ranks afterwards.
    """
    item_filter = check_item_filter_early(item_filter, Q)
    P, Q, item_bias, U, I, d = tables(P, Q, item_bias)
    item_filter = check_item_filter(item_filter, I)
    users = int32_ids(users, strict=True)
    n = users.numel()
    if tgt_indptr.dtype != torch.int64 or tgt_items.dtype != torch.int32:
        raise ValueError("tgt_indptr must be int64 and tgt_items int32")
    if tgt_indptr.dim() != 1 or tgt_indptr.numel() != n + 1:
        raise ValueError("tgt_indptr must have n+1 entries")
    seen_indptr, seen_indices = seen_csr(seen_indptr, seen_indices, U)
    # (the shapes are checked on any device; the work is not done on any)
    need_rocm("rank_items", "the tables, the rows and the targets", (P, Q, users, tgt_indptr, tgt_items, item_filter),
              (P, Q, item_bias, users, tgt_indptr, tgt_items, seen_indptr, seen_indices, item_filter), "P")
    native.load()
    dev = P.device
    tgt_indptr, tgt_items = tgt_indptr.contiguous(), tgt_items.reshape(-1).contiguous()
    total = tgt_items.numel()
    rank = torch.full((total,), -1, dtype=torch.int32, device=dev)
    not_below = torch.full((total,), -1, dtype=torch.int32, device=dev)
    score = torch.full((total,), float("-inf"), dtype=torch.float32, device=dev)
    if n == 0:
        if total:
            raise ValueError("tgt_indptr does not describe rows of `tgt_items`")
        return rank, not_below, score
    lens = tgt_indptr[1:] - tgt_indptr[:-1]
    bad_user = ((users < 0) | (users >= U)).any() if check_users else torch.zeros((), dtype=torch.bool, device=dev)
    first, last, shortest, longest, bad_user = (int(v) for v in torch.stack(
        [tgt_indptr[0], tgt_indptr[n], lens.min(), lens.max(), bad_user.to(torch.int64)]).tolist())
    if first != 0 or shortest < 0 or last != total:
        raise ValueError("tgt_indptr does not describe rows of `tgt_items`")
    if bad_user:
        raise ValueError("user id out of range")
    if longest > RANK_TMAX:
        users, tgt_indptr = split_rows(users, tgt_indptr)
        n = users.numel()
    item_slices, ws, ws_bytes = sliced_workspace("rank", (n, I, d), item_slices, dev)
    call_rows("rank", dev,
              (P.data_ptr(), Q.data_ptr(), ptr(item_bias), I, d, users.data_ptr(), n, tgt_indptr.data_ptr(),
               tgt_items.data_ptr(), ptr(seen_indptr), ptr(seen_indices)), item_filter,
              (item_slices, ptr(ws), ws_bytes, rank.data_ptr(), not_below.data_ptr(), score.data_ptr()))
    return rank, not_below, score
