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

RANK_TMAX = 112  # bpr_rank_rows: targets of one kernel row (csrc/bpr_rank_plan.h); longer rows are split here


def workspace_bytes(n: int, num_items: int, d: int, item_slices: int = 0) -> int:
    """`bpr_rank_workspace`: bytes of device workspace a call of this shape needs."""
    out = ctypes.c_int64()
    native.check(native.load().bpr_rank_workspace(n, num_items, d, item_slices, ctypes.byref(out)))
    return int(out.value)


def slices(n: int, num_items: int, d: int, item_slices: int = 0) -> int:
    """`bpr_rank_slices`: the slice count a call of this shape runs with."""
    out = ctypes.c_int32()
    native.check(native.load().bpr_rank_slices(n, num_items, d, item_slices, ctypes.byref(out)))
    return int(out.value)


def _table(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    return t.detach().contiguous()


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
               seen_indices: Optional[torch.Tensor] = None, *, item_slices: int = 0, check_users: bool = True):
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
    """
    P, Q, item_bias = _table(P, "P"), _table(Q, "Q"), _table(item_bias, "item_bias")
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError("P [U, d] and Q [I, d] must share the embedding dim")
    (U, d), I = P.shape, Q.shape[0]
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    users = users.reshape(-1)
    n = users.numel()
    if users.dtype not in (torch.int32, torch.int64):
        raise ValueError("users must be int32 or int64")
    if tgt_indptr.dtype != torch.int64 or tgt_items.dtype != torch.int32:
        raise ValueError("tgt_indptr must be int64 and tgt_items int32")
    if tgt_indptr.dim() != 1 or tgt_indptr.numel() != n + 1:
        raise ValueError("tgt_indptr must have n+1 entries")
    if (seen_indptr is None) != (seen_indices is None):
        raise ValueError("seen_indptr and seen_indices go together")
    if seen_indptr is not None:
        if seen_indptr.dtype != torch.int64 or seen_indices.dtype != torch.int32:
            raise ValueError("seen_indptr must be int64 and seen_indices int32")
        if seen_indptr.numel() != U + 1:
            raise ValueError("seen_indptr must have U+1 entries")
    # (the shapes are checked on any device; the work is not done on any)
    if not (P.is_cuda and Q.is_cuda and users.is_cuda and tgt_indptr.is_cuda and tgt_items.is_cuda):
        raise RuntimeError("rank_items needs the tables, the rows and the targets on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != P.device
           for t in (Q, item_bias, users, tgt_indptr, tgt_items, seen_indptr, seen_indices)):
        raise RuntimeError("rank_items needs every tensor on the device of P")
    lib = native.load()
    dev = P.device
    users = users.to(torch.int32).contiguous()
    tgt_indptr, tgt_items = tgt_indptr.contiguous(), tgt_items.reshape(-1).contiguous()
    if seen_indptr is not None:
        seen_indptr, seen_indices = seen_indptr.contiguous(), seen_indices.contiguous()
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
    item_slices = slices(n, I, d, item_slices)  # the count this call runs with: the workspace is its own need
    ws_bytes = workspace_bytes(n, I, d, item_slices)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        native.check(lib.bpr_rank_rows(
            P.data_ptr(), Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d,
            users.data_ptr(), n, tgt_indptr.data_ptr(), tgt_items.data_ptr(),
            None if seen_indptr is None else seen_indptr.data_ptr(),
            None if seen_indices is None else seen_indices.data_ptr(), item_slices,
            None if ws is None else ws.data_ptr(), ws_bytes, rank.data_ptr(), not_below.data_ptr(),
            score.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return rank, not_below, score
