"""Diversified top-k on the HIP engine: greedy maximal marginal relevance (MMR) over each row's pool of candidates by
one fused kernel (`bpr_diversify_rows`, csrc/bpr_diversify.hip) — a workgroup per row keeps the pool's C x C
similarities in LDS, so there is no [n, C, d] gather and no [n, C, C] matrix.  It consumes what `recommend` /
`rerank` return ([n, C] ids and scores, -1 / -inf padding) and returns the same form.  The reference has no such
pass: it ranks through full logits (example.py:195-230).

There is no CPU path: tensors must live on a ROCm device.  `intra_list_similarity` is a metric and stays in PyTorch.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr._serving import _table, need_rocm, ptr, query
from revisit_bpr.recommend import TOPK_MAX, recommend

METRICS = {"dot": 0, "cosine": 1}   # BPR_SIM_DOT, BPR_SIM_COSINE (include/bprcore.h)
SCALES = {"none": 0, "minmax": 1}   # BPR_SCALE_NONE, BPR_SCALE_MINMAX
LAYOUT_AUTO, LAYOUT_WG = 0, 1       # `layout`: the library chooses / a workgroup per row (the only layout today)
LAYOUTS = (LAYOUT_WG,)
POOL_MAX = TOPK_MAX                 # longest pool, and largest k


def layout_of(n: int, C: int, k: int, layout: int = 0):
    """`bpr_diversify_layout`: (layout, padded C, bytes of LDS a workgroup holds) a call of this shape runs with."""
    return query("bpr_diversify_layout", n, C, k, layout, ctype=(ctypes.c_int32, ctypes.c_int32, ctypes.c_int64))


@torch.no_grad()
def diversify(Q: torch.Tensor, cand_items: torch.Tensor, cand_scores: torch.Tensor, k: int, *, lam: float = 0.7,
              metric: str = "cosine", scale: str = "none", return_mmr: bool = False, layout: int = 0):
    """Greedy MMR over each row's pool: pick the most relevant candidate, then `k - 1` times the candidate with the
    largest  lam * rel' - (1 - lam) * (its largest similarity to anything already picked).

    `cand_items` (int32) / `cand_scores` (float32) are [n, C], or 1-D for one row, C <= 128: what `recommend` and
    `rerank` return goes in unchanged.  A candidate is eligible if 0 < id < I and its relevance is finite (the
    -1 / -inf padding, id 0 and NaN drop out); an id listed twice is two candidates.  `metric`: "cosine" or "dot"
    between the rows of `Q` [I, d].  `scale`: "none" uses the relevances as given, "minmax" maps each row's eligible
    relevances onto [0, 1] first (what makes `lam` mean the same across users); the scores returned are the
    original ones either way.  lam = 1 is the pool sorted by (score desc, id asc); lam = 0 is pure dispersion.

    Returns (items [n, k] int32, scores [n, k] float32) in pick order, a row with fewer than k eligible candidates
    ending in -1 / -inf; `return_mmr=True` adds the objective each pick won with ([n, k] float32, -inf padding).
    Ties go to the larger relevance, then the smaller id: the result does not depend on n, on the order of the rows,
    on the order of the candidates inside a row or on `layout`.  The arithmetic is defined bit for bit in
    include/bprcore.h.  Nothing is read back: the call runs on the current stream and can be captured.
    """
    k = int(k)
    if k > POOL_MAX:
        raise ValueError(f"k = {k}: diversify returns at most {POOL_MAX} items per row")
    if k < 0:
        raise ValueError("k must be at least 0")
    lam = float(lam)
    if not (0.0 <= lam <= 1.0) or math.isnan(lam):
        raise ValueError(f"lam = {lam}: must be in [0, 1]")
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}: 'cosine' or 'dot'")
    if scale not in SCALES:
        raise ValueError(f"unknown scale {scale!r}: 'none' or 'minmax'")
    if layout not in (LAYOUT_AUTO,) + LAYOUTS:
        raise ValueError(f"layout must be 0 (choose) or {LAYOUT_WG} (workgroup per row)")
    Q = _table(Q, "Q")
    if Q.dim() != 2:
        raise ValueError("Q must be [I, d]")
    I, d = Q.shape
    if cand_items.dtype != torch.int32:
        raise ValueError("cand_items must be int32")
    if cand_scores.dtype != torch.float32:
        raise ValueError("cand_scores must be float32")
    if cand_items.shape != cand_scores.shape:
        raise ValueError("cand_items and cand_scores must have the same shape")
    if cand_items.dim() not in (1, 2):
        raise ValueError("cand_items must be [n, C], or 1-D for one row")
    one = cand_items.dim() == 1
    if one:
        cand_items, cand_scores = cand_items.unsqueeze(0), cand_scores.unsqueeze(0)
    n, C = cand_items.shape
    if C < 1 or C > POOL_MAX:
        raise ValueError(f"C = {C}: a pool holds 1 to {POOL_MAX} candidates")
    cand_items, cand_scores = cand_items.contiguous(), cand_scores.detach().contiguous()
    # (the arguments are checked on any device; the work is not done on any)
    need_rocm("diversify", "the item table and the candidates", (Q, cand_items, cand_scores),
              (Q, cand_items, cand_scores), "Q")
    dev = Q.device
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    mmr = torch.empty((n, k), dtype=torch.float32, device=dev) if return_mmr else None
    if n and k:
        with torch.cuda.device(dev):
            native.check(native.load().bpr_diversify_rows(
                Q.data_ptr(), I, d, cand_items.data_ptr(), cand_scores.data_ptr(), n, C, k, lam, METRICS[metric],
                SCALES[scale], layout, items.data_ptr(), scores.data_ptr(), ptr(mmr),
                torch.cuda.current_stream(dev).cuda_stream))
    if one:
        items, scores, mmr = items[0], scores[0], None if mmr is None else mmr[0]
    return (items, scores, mmr) if return_mmr else (items, scores)


@torch.no_grad()
def recommend_diverse(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor, k: int,
                      *, pool: int = 100, lam: float = 0.7, metric: str = "cosine", scale: str = "minmax",
                      seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None,
                      check_users: bool = True, item_filter: Optional[torch.Tensor] = None):
    """`recommend(pool)` followed by `diversify(k)`: the `k` picks of greedy MMR from every user's `pool` best unseen
    items.  (items [n, k] int32, scores [n, k] float32), the scores being `recommend`'s.  lam = 1 returns
    `recommend(k)` bit for bit.  `item_filter` is `recommend`'s: the pool holds eligible items only."""
    k, pool = int(k), int(pool)
    if pool < k:
        raise ValueError(f"pool = {pool} is shorter than k = {k}")
    if pool > POOL_MAX:
        raise ValueError(f"pool = {pool}: a pool holds at most {POOL_MAX} candidates")
    cand, rel = recommend(P, Q, item_bias, users, pool, seen_indptr, seen_indices, check_users=check_users,
                          item_filter=item_filter)
    return diversify(Q, cand, rel, k, lam=lam, metric=metric, scale=scale)


@torch.no_grad()
def intra_list_similarity(Q: torch.Tensor, items: torch.Tensor, metric: str = "cosine",
                          block_bytes: int = 1 << 28) -> torch.Tensor:
    """Mean pairwise similarity of each returned list ([n, k] ids, -1 = padding, ignored): float32 [n], 0 for a list
    with fewer than two items.  Plain blocked PyTorch, on whatever device the tensors live on: a metric, not a hot
    path.  Low is diverse."""
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}: 'cosine' or 'dot'")
    if items.dim() == 1:
        items = items.unsqueeze(0)
    n, k = items.shape
    d = Q.shape[1]
    out = torch.zeros(n, dtype=torch.float32, device=Q.device)
    step = max(1, block_bytes // max(1, 4 * k * (d + k)))
    for lo in range(0, n, step):
        ids = items[lo:lo + step].long()
        live = ids >= 0
        X = Q[ids.clamp(min=0)].float() * live.unsqueeze(-1)
        if metric == "cosine":
            X = X / X.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        S = torch.bmm(X, X.transpose(1, 2))
        pair = live.unsqueeze(1) & live.unsqueeze(2)
        pair &= ~torch.eye(k, dtype=torch.bool, device=Q.device)
        cnt = pair.sum((1, 2))
        out[lo:lo + step] = (S * pair).sum((1, 2)) / cnt.clamp_min(1)
    return out
