"""Re-ranking on the HIP engine: every row — a user and a list of candidate items — scored on its own candidates
and cut to its k best by one fused gather kernel (`bpr_rerank_rows`, csrc/bpr_rerank.hip), with no [nnz, d] buffer
and no sweep of the item table.  Availability filters, second-stage re-ranking, sampled-negative protocols and
explicit (user, item) pairs are this one call.  The scores are `recommend`'s and `rank_items`' bits.  The reference
has no candidate path: it ranks through full logits (example.py:195-230).

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr._serving import int32_ids, need_rocm, ptr, query, seen_csr, tables
from revisit_bpr.recommend import TOPK_MAX

LAYOUT_AUTO, LAYOUT_WAVE, LAYOUT_WG = 0, 1, 2  # `layout`: the library chooses / a wave per row / a workgroup per row
LAYOUTS = (LAYOUT_WAVE, LAYOUT_WG)
RERANK_TILE = 256  # csrc/bpr_rerank_plan.h: candidates the workgroup layout stages at a time (the wave layout: 64)


def layout_of(n: int, d: int, k: int, row_len: int, layout: int = 0):
    """`bpr_rerank_layout`: (layout, tile) a call of this shape runs with; `row_len` is the length of the shared
    list or the mean length of the CSR rows."""
    return query("bpr_rerank_layout", n, d, k, row_len, layout, ctype=(ctypes.c_int32, ctypes.c_int32))


@torch.no_grad()
def rerank(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor,
           cand_items: torch.Tensor, k: int, cand_indptr: Optional[torch.Tensor] = None,
           seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None, *,
           return_scores: bool = False, layout: int = 0, check_users: bool = True):
    """The `k` best of each row's OWN candidates by <P[u], Q[i]> (+ item_bias[i]).  Row r is user `users[r]` with
    the candidates `cand_items[cand_indptr[r]:cand_indptr[r + 1]]` (int64 [n + 1] starting at 0, int32; unsorted,
    duplicates allowed, any length) or, for a 1-D `cand_items` without `cand_indptr`, that one list for every row.
    A candidate is eligible if 0 < id < I and it is not in the user's row of the seen CSR (int64 [U+1], int32
    sorted per row; None: nothing is seen).

    Returns (items [n, k] int32, scores [n, k] float32): rows sorted by score descending, ties by ascending item
    id, an id listed m times returned up to m times, adjacent; a row with fewer than k eligible candidates ends in
    item -1 / score -inf.  `return_scores=True` adds cand_scores (float32, aligned with `cand_items`; [n, C] for
    the shared list): every candidate's score, -inf for an ineligible one.  A score is the bits `recommend` and
    `rank_items` return for the pair.
    A NaN score (a NaN in a row, 0 * inf, inf - inf) is never returned, so such a row may end in padding although
    candidates are left, and cand_scores holds it as it is; +inf and -inf scores are ordered like any other, and a
    real item scoring -inf keeps its id: only the padding is item -1 (tests/test_gpu_chain.py).
    The result does not depend on n, on the order of the rows, on the order of
    the candidates inside a row or on `layout` (0: the library chooses; LAYOUT_WAVE, LAYOUT_WG).  Runs on the
    current stream.  The kernel reads P[user], the user's CSR row and `cand_indptr` unchecked, so they are checked
    here first, which waits for the device; `check_users=False` leaves that out.
    """
    k = int(k)
    if k > TOPK_MAX:
        raise ValueError(f"k = {k}: rerank returns at most {TOPK_MAX} items per row")
    if k < 0:
        raise ValueError("k must be at least 0")
    if k == 0 and not return_scores:
        raise ValueError("k = 0 returns nothing without return_scores (score_candidates)")
    if layout not in (LAYOUT_AUTO,) + LAYOUTS:
        raise ValueError(f"layout must be 0 (choose), {LAYOUT_WAVE} (wave per row) or {LAYOUT_WG} (workgroup per row)")
    P, Q, item_bias, U, I, d = tables(P, Q, item_bias)
    users = int32_ids(users, strict=True)
    n = users.numel()
    if cand_items.dtype != torch.int32:
        raise ValueError("cand_items must be int32")
    shared = cand_indptr is None
    if shared:
        if cand_items.dim() != 1:
            raise ValueError("cand_items without cand_indptr is ONE 1-D list shared by every row")
    else:
        if cand_indptr.dtype != torch.int64:
            raise ValueError("cand_indptr must be int64")
        if cand_indptr.dim() != 1 or cand_indptr.numel() != n + 1:
            raise ValueError("cand_indptr must have n+1 entries")
        cand_indptr = cand_indptr.contiguous()
    cand_items = cand_items.reshape(-1).contiguous()
    nnz = cand_items.numel()
    seen_indptr, seen_indices = seen_csr(seen_indptr, seen_indices, U)
    # (the arguments are checked on any device; the work is not done on any)
    need_rocm("rerank", "the tables, the user list and the candidates", (P, Q, users, cand_items, item_bias),
              (P, Q, item_bias, users, cand_items, cand_indptr, seen_indptr, seen_indices), "P")
    lib = native.load()
    dev = P.device
    if check_users and n:
        bad = [((users < 0) | (users >= U)).any()]
        if not shared:
            lens = cand_indptr[1:] - cand_indptr[:-1]
            bad.append((cand_indptr[0] != 0) | (cand_indptr[n] != nnz) | (lens.min() < 0))
        bad = torch.stack(bad).tolist()  # one wait for both answers
        if len(bad) > 1 and bad[1]:
            raise ValueError("cand_indptr does not describe rows of `cand_items`")
        if bad[0]:
            raise ValueError("user id out of range")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    cand_scores = None
    if return_scores:
        cand_scores = torch.empty((n, nnz) if shared else (nnz,), dtype=torch.float32, device=dev)
    if n == 0 and not shared and nnz:
        raise ValueError("cand_indptr does not describe rows of `cand_items`")
    if n == 0 or (k == 0 and not cand_scores.numel()):
        return (items, scores, cand_scores) if return_scores else (items, scores)
    row_len = nnz if shared else nnz // n  # the CSR's mean row: a hint to the launch plan, not an input of the result
    cand_ptr = cand_items.data_ptr() if nnz else None
    if not shared and not nnz:  # (an empty tensor has no address; every row is empty and nothing is read)
        cand_items = torch.zeros(1, dtype=torch.int32, device=dev)
        cand_ptr = cand_items.data_ptr()
    with torch.cuda.device(dev):
        native.check(lib.bpr_rerank_rows(
            P.data_ptr(), Q.data_ptr(), ptr(item_bias), I, d, users.data_ptr(), n, ptr(cand_indptr), cand_ptr, row_len,
            ptr(seen_indptr), ptr(seen_indices), k, layout,
            None if cand_scores is None or not cand_scores.numel() else cand_scores.data_ptr(),
            items.data_ptr() if k else None, scores.data_ptr() if k else None,
            torch.cuda.current_stream(dev).cuda_stream))
    return (items, scores, cand_scores) if return_scores else (items, scores)


def score_candidates(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor,
                     cand_items: torch.Tensor, cand_indptr: Optional[torch.Tensor] = None,
                     seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None, *,
                     layout: int = 0, check_users: bool = True) -> torch.Tensor:
    """`rerank` with k = 0: the score of every candidate (float32, aligned with `cand_items`; [n, C] for the shared
    list), -inf for an ineligible one, and no selection."""
    return rerank(P, Q, item_bias, users, cand_items, 0, cand_indptr, seen_indptr, seen_indices,
                  return_scores=True, layout=layout, check_users=check_users)[2]
