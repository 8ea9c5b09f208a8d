"""Fold new users into a trained model on the HIP engine: learn p_u from a new user's history against
the FROZEN item table (`bpr_fold_in_rows`, csrc/bpr_foldin.hip; with adaptive negatives
`bpr_fold_in_rows_adaptive`, csrc/bpr_foldin_adaptive.hip; with dynamic negatives or the WARP objective
`bpr_fold_in_rows_scored`, csrc/bpr_foldin_scored.hip).  The result is a [n, d] user table for
`recommend`, `evaluate_topk` and `evaluate_fused`, which take any such table plus a seen CSR.

The reference has no such step (its held-out users' histories are part of the training file,
full-train-with-fold-in.jsonl), so its configs/RQ3/user-split protocol has no BPR entry.

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr._serving import _table


def balance_order(lengths: torch.Tensor) -> torch.Tensor:
    """The order in which a fold-in launch hands out its rows: longest first (a stable descending
    argsort of the row lengths, int32), so that the rows that take longest start first."""
    return torch.argsort(lengths.reshape(-1), descending=True, stable=True).to(torch.int32)


def _check_csr(indptr: torch.Tensor, idx: torch.Tensor, idx_name: str, rows_name: str) -> None:
    if indptr.dtype != torch.int64 or idx.dtype != torch.int32:
        raise ValueError(f"indptr must be int64 and {idx_name} int32")
    if indptr.dim() != 1 or indptr.numel() < 1:
        raise ValueError(f"indptr must have {rows_name}+1 entries")


def _rows_csr(indptr: torch.Tensor, idx: torch.Tensor, idx_name: str):
    """The CSR of a fold-in call (already through `_check_csr`): (indptr, idx) contiguous, the number of rows and
    nnz — from the one host read of this wrapper, the two ends of `indptr`."""
    indptr, idx = indptr.contiguous(), idx.reshape(-1).contiguous()
    n = indptr.numel() - 1
    first, last = (int(v) for v in indptr[[0, n]].tolist())
    nnz = last - first
    if first < 0 or nnz < 0 or last > idx.numel():
        raise ValueError(f"indptr does not describe rows of `{idx_name}`")
    return indptr, idx, n, nnz


def _check_neg(neg, epochs: int, nnz: int) -> None:
    if neg is not None:
        if neg.dtype != torch.int32:
            raise ValueError("neg must be int32")
        if neg.numel() != epochs * nnz:
            raise ValueError(f"neg must have epochs * nnz = {epochs * nnz} entries")


def _initial_rows(init, init_std: float, seed: int, n: int, d: int, dev) -> torch.Tensor:
    """The rows a fold-in starts from: a copy of `init`, else N(0, init_std^2) from a generator seeded by `seed`,
    else zeros."""
    if init is not None:
        return init.detach().clone().contiguous()
    if init_std:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        return torch.randn((n, d), generator=gen, device=dev, dtype=torch.float32) * float(init_std)
    return torch.zeros((n, d), dtype=torch.float32, device=dev)


def _neg_buffers(neg, epochs: int, nnz: int, return_neg: bool, dev):
    """(neg flattened or None, the buffer of negatives used: `neg` itself, a new one to return, or None)."""
    if neg is not None:
        neg = neg.reshape(-1).contiguous()
        return neg, neg
    return None, (torch.zeros(epochs * nnz, dtype=torch.int32, device=dev) if return_neg else None)


ORDER_PAD = 4  # int32 entries that must be readable before and after `order` (include/bprcore.h)


class _PaddedOrder:
    """An `order` [d, I] that is known to have ORDER_PAD readable entries on both sides (a view into a padded
    buffer, or the engine's own snapshot): `fold_in` passes it to the kernel without a copy."""

    def __init__(self, order: torch.Tensor, keep=None) -> None:
        self.order, self.keep = order, keep


def _padded(order: torch.Tensor) -> _PaddedOrder:
    buf = torch.zeros(order.numel() + 2 * ORDER_PAD, dtype=torch.int32, device=order.device)
    view = buf[ORDER_PAD:ORDER_PAD + order.numel()].view(order.shape)
    view.copy_(order)
    return _PaddedOrder(view, buf)


@torch.no_grad()
def snapshot_of(Q: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The adaptive sampler's snapshot of an item table Q [I, d], in torch: (order [d, I] int32 — per factor every
    item id by descending q_if, ties by ascending id (a stable descending argsort over all I rows) — and sigma [d]
    float32, the unbiased std of the factor over rows 1..I-1).  sigma is computed the way `Engine.adaptive_refresh`
    computes it on the device (csrc/bpr_sort_shared.h): float64 sums of c = q_if - q_1f and of c^2 over those
    rows, sigma = sqrt(max(sum c^2 - (sum c)^2 / n, 0) / (n - 1)) with n = I - 1, rounded to float32 once."""
    if Q.dim() != 2 or Q.dtype != torch.float32:
        raise ValueError("Q must be float32 [I, d]")
    if Q.shape[0] < 3:
        raise ValueError("a snapshot needs at least two items besides the pad row")
    order = torch.argsort(Q.detach().t().contiguous(), dim=1, descending=True, stable=True).to(torch.int32)
    c = Q.detach()[1:].double() - Q.detach()[1].double()  # shifted by row 1: the mean's magnitude leaves the sums
    n = float(Q.shape[0] - 1)
    a, b = c.sum(dim=0), (c * c).sum(dim=0)
    sigma = torch.sqrt(torch.clamp(b - a * a / n, min=0.0) / (n - 1.0)).float()
    return order.contiguous(), sigma.contiguous()


@torch.no_grad()
def fold_in(Q: torch.Tensor, item_bias: Optional[torch.Tensor], indptr: torch.Tensor, items: torch.Tensor, *,
            epochs: int, lr: float, reg_user: float = 0.0, init: Optional[torch.Tensor] = None,
            init_std: float = 0.0, seed: int = 0, offset: int = 0, neg: Optional[torch.Tensor] = None,
            return_neg: bool = False, balance: bool = True, sampler: str = "uniform", adaptive_p: float = 0.01,
            snapshot: Optional[tuple] = None, return_draws: bool = False, candidates: int = 4,
            max_sampled: int = 10, margin: float = 1.0, _seen_mode: int = 0, _states: bool = False):
    """User rows P_new [n, d] for the n new users whose histories are the rows of the CSR (`indptr`
    int64 [n+1], `items` int32, sorted per row, no duplicates, ids in [1, I)), learnt by `epochs`
    sequential BPR-SGD passes over each history against the frozen `Q` [I, d] (+ `item_bias` [I]):

        x = <p, q_i - q_j> (+ b_i - b_j),  w = sigma(-x),  p <- p - lr (-w (q_i - q_j) + reg_user p)

    Negatives: `neg` (int32, exactly epochs * nnz entries, entry e * nnz + k belongs to epoch e and CSR
    position k) or, with `neg=None`, drawn on the device uniformly over the items the user has not seen
    — the draw of `Engine.sample_uniform` for counter `offset` + that index under `seed`.  A negative 0
    skips its triple (a user who has seen every item keeps the initial row).  `init`: the initial rows
    (copied); None: zeros, or N(0, init_std^2) from a `torch.Generator` seeded by `seed`.  `balance`:
    rows are handed to the kernel longest first (it changes the time, never the result).
    `return_neg=True` returns (P_new, negatives used).  Runs on the current stream, and waits for it
    TWICE before the launch: this wrapper reads the two ends of `indptr` to size and check `neg`, and
    `bpr_fold_in_rows` reads them again for its own bound (it takes no nnz argument).

    `sampler="adaptive"` (`neg` must be None): the negative of a triple is `Engine.sample_adaptive`'s draw for
    counter `offset` + that index under `seed` and `adaptive_p`, for a user whose row is the row as it stands
    just before that triple's update and whose seen items are this history, from `snapshot` = (order [d, I]
    int32, sigma [d] float32) of the item table; None: `snapshot_of(Q)`.  `return_draws=True` appends the
    (factor, rank) pairs: (P_new[, negatives], factors, ranks), int32 [epochs * nnz] each.

    `sampler="dynamic"` / `sampler="warp"` (`neg` must be None; `bpr_fold_in_rows_scored`): fold in with the sampler
    the table was trained with.  The draw of a triple is `Engine.sample_dynamic`'s (the highest-scoring of the first
    `candidates` unseen candidates, 1 .. 32) or `Engine.sample_warp`'s (the first of at most `max_sampled`, 1 .. 32,
    that scores above the positive's score less `margin`, finite and > 0) for counter `offset` + that index under
    `seed`, for a user whose row is the row as it stands just before that triple's update and whose seen items are
    this history.  "dynamic" takes the step above with the pick.  "warp" takes the step of the WARP objective,
    p <- p - lr (-L (q_i - q_j) + reg_user p) with L = log(max(1, floor(n_unseen / tries))), n_unseen = (I - 1) - the
    history's length, and SKIPS a triple without a violator (no step, not even the L2 term): its negative is -1.
    `return_neg=True` returns the picks; `return_draws=True` appends `tries`, int32 [epochs * nnz]: under "warp" the
    number of the candidate that violated (0 = skipped), under "dynamic" zeros (that draw looks at all its
    candidates and counts nothing).  `snapshot` and `adaptive_p` stay adaptive-only.
    """
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError("epochs must be at least 1")
    if sampler not in ("uniform", "adaptive", "dynamic", "warp"):
        raise ValueError("sampler must be 'uniform', 'adaptive', 'dynamic' or 'warp'")
    adaptive, scored = sampler == "adaptive", sampler in ("dynamic", "warp")
    if (adaptive or scored) and neg is not None:
        raise ValueError(f"given negatives (`neg`) and sampler='{sampler}' exclude each other")
    if adaptive and not 0.0 < float(adaptive_p) < 1.0:
        raise ValueError("adaptive_p must be in (0, 1)")
    if sampler == "dynamic" and not 1 <= int(candidates) <= 32:
        raise ValueError("candidates must be in [1, 32]")
    if sampler == "warp" and not 1 <= int(max_sampled) <= 32:
        raise ValueError("max_sampled must be in [1, 32]")
    if sampler == "warp" and not (math.isfinite(float(margin)) and float(margin) > 0.0):
        raise ValueError("margin must be finite and > 0")
    if return_draws and not (adaptive or scored):
        raise ValueError("return_draws needs sampler='adaptive', 'dynamic' or 'warp'")
    if _states and not scored:
        raise ValueError("_states needs sampler='dynamic' or 'warp'")
    if snapshot is not None and not adaptive:
        raise ValueError("snapshot needs sampler='adaptive'")
    Q, item_bias = _table(Q, "Q"), _table(item_bias, "item_bias")
    if Q.dim() != 2:
        raise ValueError("Q must be [I, d]")
    I, d = Q.shape
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    _check_csr(indptr, items, "items", "n")
    indptr, items, n, nnz = _rows_csr(indptr, items, "items")
    dev = Q.device
    if init is not None and (init.dtype != torch.float32 or tuple(init.shape) != (n, d)):
        raise ValueError("init must be float32 [n, d]")
    _check_neg(neg, epochs, nnz)
    padded = None
    if snapshot is not None:
        order, sigma = snapshot
        padded = order if isinstance(order, _PaddedOrder) else None
        order = padded.order if padded is not None else order
        if order.dtype != torch.int32 or sigma.dtype != torch.float32:
            raise ValueError("snapshot must be (order int32, sigma float32)")
        if tuple(order.shape) != (d, I) or tuple(sigma.shape) != (d,):
            raise ValueError("snapshot must be (order [d, I], sigma [d])")
    # (the shapes are checked on any device; the work is not done on any)
    if not (Q.is_cuda and indptr.is_cuda and items.is_cuda):
        raise RuntimeError("fold_in needs the item table and the histories on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != Q.device for t in (item_bias, indptr, items, init, neg)):
        raise RuntimeError("fold_in needs every tensor on the device of Q")
    if snapshot is not None and (order.device != Q.device or sigma.device != Q.device):
        raise RuntimeError("fold_in needs every tensor on the device of Q")
    lib = native.load()
    P_new = _initial_rows(init, init_std, seed, n, d, dev)
    neg, used = _neg_buffers(neg, epochs, nnz, return_neg, dev)
    fac = rnk = tries = states = None
    if scored:
        if return_draws:
            tries = torch.zeros(epochs * nnz, dtype=torch.int32, device=dev)
        if _states:
            states = torch.zeros((epochs * nnz, d), dtype=torch.float32, device=dev)
    elif return_draws:
        fac = torch.zeros(epochs * nnz, dtype=torch.int32, device=dev)
        rnk = torch.zeros(epochs * nnz, dtype=torch.int32, device=dev)
    if adaptive and n and nnz:
        if snapshot is None:
            order, sigma = snapshot_of(Q)
        if padded is None or not order.is_contiguous():
            padded = _padded(order)
        sigma = sigma.contiguous()
        rows = balance_order(indptr[1:] - indptr[:-1]) if balance else None
        fn, tail = lib.bpr_fold_in_rows_adaptive, ()
        if _seen_mode:  # tests: the library's launch entry with the seen structure forced (1 CSR, 2 bitmap)
            fn, tail = lib.bpr_test_fold_in_rows_adaptive, (int(_seen_mode),)
            fn.restype, fn.argtypes = ctypes.c_int, native.SIGNATURES["bpr_fold_in_rows_adaptive"][1] + [ctypes.c_int32]
        with torch.cuda.device(dev):
            native.check(fn(
                Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d, padded.order.data_ptr(),
                sigma.data_ptr(), indptr.data_ptr(), items.data_ptr(), n, None if rows is None else rows.data_ptr(),
                epochs, float(lr), float(reg_user), float(adaptive_p), None if used is None else used.data_ptr(),
                None if fac is None else fac.data_ptr(), None if rnk is None else rnk.data_ptr(), int(seed),
                int(offset), P_new.data_ptr(), torch.cuda.current_stream(dev).cuda_stream, *tail))
    elif scored and n and nnz:
        rows = balance_order(indptr[1:] - indptr[:-1]) if balance else None
        warp = sampler == "warp"
        fn, tail = lib.bpr_fold_in_rows_scored, ()
        if _seen_mode or _states:  # tests: the seen structure forced (1 CSR, 2 bitmap), the row each draw saw
            fn = lib.bpr_test_fold_in_rows_scored
            tail = (int(_seen_mode), None if states is None else states.data_ptr())
            fn.restype = ctypes.c_int
            fn.argtypes = native.SIGNATURES["bpr_fold_in_rows_scored"][1] + [ctypes.c_int32, ctypes.c_void_p]
        with torch.cuda.device(dev):
            native.check(fn(
                Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d, indptr.data_ptr(),
                items.data_ptr(), n, None if rows is None else rows.data_ptr(), epochs, float(lr), float(reg_user),
                native.NEG_WARP if warp else native.NEG_DYNAMIC, int(max_sampled if warp else candidates),
                float(margin), None if used is None else used.data_ptr(),
                None if tries is None else tries.data_ptr(), int(seed), int(offset), P_new.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream, *tail))
    elif n and nnz:
        order = balance_order(indptr[1:] - indptr[:-1]) if balance else None
        with torch.cuda.device(dev):
            native.check(lib.bpr_fold_in_rows(
                Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d, indptr.data_ptr(),
                items.data_ptr(), n, None if order is None else order.data_ptr(), epochs, float(lr),
                float(reg_user), native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM,
                None if neg is None else neg.data_ptr(),
                None if (neg is not None or used is None) else used.data_ptr(), int(seed), int(offset),
                P_new.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    draws = ((tries,) if scored else (fac, rnk)) if return_draws else ()
    out = (P_new,) + ((used,) if return_neg else ()) + draws + ((states,) if _states else ())
    return out if len(out) > 1 else P_new
