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
from revisit_bpr.recommend import _table

SAMPLE_MAX = 128  # bpr_sample_rows: largest k


def workspace_bytes(n: int, num_items: int, d: int, k: int, item_slices: int = 0, want_log_z: bool = False) -> int:
    """`bpr_sample_workspace`: bytes of device workspace a call of this shape needs."""
    out = ctypes.c_int64()
    native.check(native.load().bpr_sample_workspace(n, num_items, d, k, item_slices, int(bool(want_log_z)),
                                                    ctypes.byref(out)))
    return int(out.value)


def slices(n: int, num_items: int, d: int, k: int, item_slices: int = 0) -> int:
    """`bpr_sample_slices`: the slice count a call of this shape runs with."""
    out = ctypes.c_int32()
    native.check(native.load().bpr_sample_slices(n, num_items, d, k, item_slices, ctypes.byref(out)))
    return int(out.value)


@torch.no_grad()
def sample_items(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], users: torch.Tensor, k: int,
                 seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None, *,
                 temperature: float = 1.0, seed: int = 0, draw_ids: Optional[torch.Tensor] = None,
                 return_keys: bool = False, return_log_z: bool = False, item_slices: int = 0,
                 check_users: bool = True):
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
    if not (P.is_cuda and Q.is_cuda and users.is_cuda and (item_bias is None or item_bias.is_cuda)):
        raise RuntimeError("sample_items needs the tables and the user list on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != P.device
           for t in (Q, item_bias, users, seen_indptr, seen_indices, draw_ids)):
        raise RuntimeError("sample_items needs every tensor on the device of P")
    lib = native.load()
    P, Q, item_bias = _table(P, "P"), _table(Q, "Q"), _table(item_bias, "item_bias")
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError("P [U, d] and Q [I, d] must share the embedding dim")
    (U, d), I = P.shape, Q.shape[0]
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    dev = P.device
    if users.dtype not in (torch.int32, torch.int64):
        raise ValueError("users must be int32 or int64")
    users = users.reshape(-1)
    if users.dtype != torch.int32:
        users = users.to(torch.int32)
    users = users.contiguous()
    n = users.numel()
    if draw_ids is not None:
        if draw_ids.dtype != torch.int64:
            raise ValueError("draw_ids must be int64")
        draw_ids = draw_ids.reshape(-1).contiguous()
        if draw_ids.numel() != n:
            raise ValueError("draw_ids must have one entry per row of users")
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
    keys = torch.empty((n, k), dtype=torch.float32, device=dev) if return_keys else None
    log_z = torch.empty(n, dtype=torch.float32, device=dev) if return_log_z else None
    item_slices = slices(n, I, d, k, item_slices)  # the count this call runs with: the workspace is its own need
    ws_bytes = workspace_bytes(n, I, d, k, item_slices, return_log_z)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev) if ws_bytes else None
    with torch.cuda.device(dev):
        native.check(lib.bpr_sample_rows(
            P.data_ptr(), Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d,
            users.data_ptr(), n, None if draw_ids is None else draw_ids.data_ptr(),
            None if seen_indptr is None else seen_indptr.data_ptr(),
            None if seen_indices is None else seen_indices.data_ptr(), k, temperature, seed, item_slices,
            None if ws is None else ws.data_ptr(), ws_bytes, items.data_ptr(), scores.data_ptr(),
            None if keys is None else keys.data_ptr(), None if log_z is None else log_z.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream))
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
