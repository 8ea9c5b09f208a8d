"""Sampling on the HIP engine: k unseen items per user drawn without replacement from softmax(score / T)
over the user's eligible items — the Plackett-Luce model — from one fused kernel (`bpr_sample_rows`,
csrc/bpr_sample.hip), with no [n, I] score matrix.  A recommender that only shows its arg-max never learns
about anything else, and its logs cannot be used for off-policy evaluation; this is `recommend` with
exploration, and `log_propensity` gives what a log needs.

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from revisit_bpr import native
from revisit_bpr.item_filter import check_item_filter, check_item_filter_early
from revisit_bpr._serving import call_rows, int32_ids, need_rocm, ptr, query, seen_csr, sliced_workspace, tables

SAMPLE_MAX = 128  # bpr_sample_rows: largest k


def workspace_bytes(n: int, num_items: int, d: int, k: int, item_slices: int = 0, want_log_z: bool = False) -> int:
    """`bpr_sample_workspace`: bytes of device workspace a call of this shape needs."""
    return query("bpr_sample_workspace", n, num_items, d, k, item_slices, int(bool(want_log_z)), ctype=ctypes.c_int64)


def slices(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_sample_slices`: the slice count a call of this shape runs with."""
    return query("bpr_sample_slices", n, num_items, d, k, item_slices)


@torch.no_grad()
def sample_items(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor, k: int,
                 seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None, *,
                 temperature: float = 1.0, seed: int = 0, draw_ids: Optional[torch.Tensor] = None,
                 return_keys: bool = False, return_log_z: bool = False, item_slices: int = 0,
                 check_users: bool = True, item_filter: Optional[torch.Tensor] = None):
    """`k` items per user of `users`, drawn without replacement from softmax(s(u, .) / temperature) over the
    user's eligible items, s(u, i) = <P[u], Q[i]> (+ item_bias[i]) with `recommend`'s bits; item 0 and the
    user's row of the seen CSR (int64 [U+1], int32 sorted per row; None: only item 0) are left out.

    Returns (items [n, k] int32, scores [n, k] float32[, keys [n, k] float32][, log_z [n] float32]).  Rows
    are in draw order, that is, by key descending (key = score / T + Gumbel noise), ties by ascending id;
    `scores` are the unperturbed scores of the drawn items.  A row with fewer than k eligible items ends in
    item -1 / score -inf / key -inf.  A NaN score is never drawn; a +inf score is drawn first.
    `log_z` is log sum exp(score / T) over the row's eligible items (`log_propensity` takes it).

    The draw is counter-based: a row's result is a pure function of the tables, the user, the row's
    `draw_ids` entry (int64 [n]; None: the user id), `seed` and `temperature` — not of n, of the order of
    `users` or of `item_slices` (log_z is held to a tolerance, and its last bits may depend on
    `item_slices`).  The same user twice with the same draw id is the same row twice: give rows distinct
    draw ids, a request counter for instance, for independent draws.  `check_users` as in `recommend`.

    `item_filter` (None: the whole catalogue): a packed filter of `revisit_bpr.item_filter.pack_item_filter` over
    the I items, on the tables' device; the draw is over the items whose bit is set, and `log_z` normalises over
    them alone, so that `log_propensity` is the propensity of a draw from the restricted catalogue
    (`bpr_sample_rows_filtered`).  An item's noise does not depend on the filter: an eligible item has the key it
    has without one.
    """
    k = int(k)
    if k > SAMPLE_MAX:
        raise ValueError(f"k = {k}: sample_items returns at most {SAMPLE_MAX} items per user")
    if k < 1:
        raise ValueError("k must be at least 1")
    temperature = float(temperature)
    with np.errstate(all="ignore"):
        inv_temp = np.float32(1.0) / np.float32(temperature)
    if not (math.isfinite(temperature) and temperature > 0 and np.isfinite(np.float32(temperature))
            and np.isfinite(inv_temp) and np.float32(temperature) > 0):
        raise ValueError("temperature must be finite and > 0 in float32, and so must 1 / temperature")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    item_filter = check_item_filter_early(item_filter, Q)
    need_rocm("sample_items", "the tables and the user list", (P, Q, users, item_bias, item_filter),
              (P, Q, item_bias, users, seen_indptr, seen_indices, draw_ids, item_filter), "P")
    native.load()
    P, Q, item_bias, U, I, d = tables(P, Q, item_bias)
    item_filter = check_item_filter(item_filter, I)
    dev = P.device
    users = int32_ids(users, strict=True)
    n = users.numel()
    if draw_ids is not None:
        if draw_ids.dtype != torch.int64:
            raise ValueError("draw_ids must be int64")
        draw_ids = draw_ids.reshape(-1).contiguous()
        if draw_ids.numel() != n:
            raise ValueError("draw_ids must have one entry per row of users")
    seen_indptr, seen_indices = seen_csr(seen_indptr, seen_indices, U)
    if check_users and n and bool(((users < 0) | (users >= U)).any()):
        raise ValueError("user id out of range")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    keys = torch.empty((n, k), dtype=torch.float32, device=dev) if return_keys else None
    log_z = torch.empty(n, dtype=torch.float32, device=dev) if return_log_z else None
    item_slices, ws, ws_bytes = sliced_workspace("sample", (n, I, d, k), item_slices, dev,
                                                 post=(int(bool(return_log_z)),), words=True)
    call_rows("sample", dev,
              (P.data_ptr(), Q.data_ptr(), ptr(item_bias), I, d, users.data_ptr(), n, ptr(draw_ids), ptr(seen_indptr),
               ptr(seen_indices)), item_filter,
              (k, temperature, seed, item_slices, ptr(ws), ws_bytes, items.data_ptr(), scores.data_ptr(), ptr(keys),
               ptr(log_z)))
    out = (items, scores)
    if return_keys:
        out += (keys,)
    if return_log_z:
        out += (log_z,)
    return out


def log_propensity(scores: torch.Tensor, log_z: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """The Plackett-Luce log-probability of every returned prefix's last draw: at position j,
    score_j / T - log(exp(log_z) - sum_{m<j} exp(score_m / T)) — the log-probability that item j was drawn
    given the j items before it; their running sum along a row is the log-probability of the prefix as an
    ordered list.  `scores` [n, k] and `log_z` [n] as `sample_items` returns them.  Plain torch (O(n k)),
    in float64, relative to log_z so that nothing overflows: log(1 - sum_{m<j} exp(score_m / T - log_z)).
    Padding (score -inf) gives -inf; where the drawn items have exhausted the mass in floating point the
    result is nan-free but meaningless, as the inputs are.  Returns float64 [n, k]."""
    x = scores.to(torch.float64) / float(temperature) - log_z.to(torch.float64).unsqueeze(1)  # log p_j, <= 0
    p = torch.exp(x)
    before = torch.cumsum(p, dim=1) - p
    rest = torch.clamp(1.0 - before, min=torch.finfo(torch.float64).tiny)
    return x - torch.log(rest)
