"""Fold new items into a trained model on the HIP engine: learn q_i (and b_i) of an item that enters the
catalogue after training from the list of users who interacted with it, against the FROZEN user table,
item table and item bias (`bpr_fold_in_item_rows`, csrc/bpr_foldin_items.hip; with `neg_role`, in both
roles: `bpr_fold_in_item_rows_roles`, csrc/bpr_foldin_items_roles.hip).  The mirror image of
`revisit_bpr.foldin.fold_in`.  The result is a [m, d] block of item rows (and [m] biases):
`torch.cat((Q, Q_new))` and `torch.cat((item_bias, bias_new))` go straight into `recommend`, `rank_items`
and the evaluators, where the new items have the ids I, I + 1, ...

The reference has no such step: its time-split and user-split protocols put every item into the training
file.

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr._serving import _table, seen_csr
from revisit_bpr.foldin import _check_csr, _check_neg, _initial_rows, _neg_buffers, _rows_csr, balance_order


@torch.no_grad()
def fold_in_items(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor], indptr: torch.Tensor,
                  users: torch.Tensor, *, epochs: int, lr: float, reg_item: float = 0.0,
                  seen_indptr: Optional[torch.Tensor] = None, seen_indices: Optional[torch.Tensor] = None,
                  init: Optional[torch.Tensor] = None, init_bias: Optional[torch.Tensor] = None,
                  init_std: float = 0.0, seed: int = 0, offset: int = 0, neg: Optional[torch.Tensor] = None,
                  return_neg: bool = False, balance: bool = True, neg_role=0,
                  train_users: Optional[torch.Tensor] = None, train_items: Optional[torch.Tensor] = None,
                  return_roles: bool = False):
    """Item rows Q_new [m, d] for the m new items whose audiences are the rows of the CSR (`indptr` int64
    [m+1], `users` int32, sorted per row, no duplicates, ids in [0, U)), learnt by `epochs` sequential
    BPR-SGD passes over each audience against the frozen `P` [U, d], `Q` [I, d] (+ `item_bias` [I]):

        x = <p_u, q - q_j> (+ b - b_j),  w = sigma(-x),  q <- q - lr (-w p_u + reg_item q),  b <- b + lr w

    Returns Q_new, or (Q_new, bias_new [m]) when `item_bias` is given; `return_neg=True` appends the
    negatives used.  Nothing is changed in place: the rows are returned, and `torch.cat((Q, Q_new))` with
    `torch.cat((item_bias, bias_new))` go straight into `recommend`, `rank_items` and `evaluate_*`.

    Negatives: `neg` (int32, exactly epochs * nnz entries, entry e * nnz + k belongs to epoch e and CSR
    position k) or, with `neg=None`, drawn on the device uniformly over the items of `Q` that the triple's
    USER has not seen according to the CSR (`seen_indptr` int64 [U+1], `seen_indices` int32; both None:
    nothing is seen) — the draw of `Engine.sample_uniform` for that user at counter `offset` + that index
    under `seed`.  A new item is never a negative.  A negative 0 skips its triple (a user who has seen every
    item teaches the new item nothing).  `init` / `init_bias`: the initial rows / biases (copied); None:
    zeros, or for the rows N(0, init_std^2) from a `torch.Generator` seeded by `seed`.  `balance`: rows are
    handed to the kernel longest first (it changes the time, never the result).  Runs on the current stream,
    and waits for it TWICE before the launch: this wrapper reads the two ends of `indptr` to size and check
    `neg`, and `bpr_fold_in_item_rows` reads them again for its own bound.

    `neg_role` (R): besides being the positive of its audience, each new item is the NEGATIVE of R training
    interactions per epoch — triples (u, i, new) with (u, i) drawn from `train_users` / `train_items` (int32,
    equal length T, the arrays the trainers take) among users outside the item's audience, spread evenly
    between the audience's steps: x = <p_u, q_i - q> (+ b_i - b), w = sigma(-x), q <- q - lr (w p_u +
    reg_item q), b <- b - lr w.  These are the updates joint training gives every item about T / I times an
    epoch; without them a folded-in item is only ever pushed up and, with more epochs, outranks warm items
    for everybody.  0 (the default): none, the call above.  An int: R.  "auto": max(1, round(T / (I - 1))),
    the expected count under joint uniform training.  A row without an audience then still takes its R
    steps.  `return_roles=True` appends the int32 [epochs * m * R] indices into the training arrays that
    were used (entry (e * m + r) * R + rho; -1: no interaction outside the audience was found in 16 draws,
    the step was skipped).  The draws are a function of (`seed`, `offset`, that entry) alone.
    """
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError("epochs must be at least 1")
    P, Q, item_bias = _table(P, "P"), _table(Q, "Q"), _table(item_bias, "item_bias")
    if Q.dim() != 2 or P.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError("P must be [U, d] and Q [I, d]")
    (U, d), I = P.shape, Q.shape[0]
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    _check_csr(indptr, users, "users", "m")
    seen_indptr, seen_indices = seen_csr(seen_indptr, seen_indices, U, flat=True,
                                         together="seen_indptr and seen_indices must both be given or both be None")
    indptr, users, m, nnz = _rows_csr(indptr, users, "users")
    dev = Q.device
    if init is not None and (init.dtype != torch.float32 or tuple(init.shape) != (m, d)):
        raise ValueError("init must be float32 [m, d]")
    if init_bias is not None:
        if item_bias is None:
            raise ValueError("init_bias needs item_bias")
        if init_bias.dtype != torch.float32 or tuple(init_bias.shape) != (m,):
            raise ValueError("init_bias must be float32 [m]")
    _check_neg(neg, epochs, nnz)
    R, train_users, train_items = _roles(neg_role, train_users, train_items, I)
    if epochs * m * R >= 2 ** 31:
        raise ValueError("epochs * m * neg_role must be below 2^31")
    # (the shapes are checked on any device; the work is not done on any)
    if not (P.is_cuda and Q.is_cuda and indptr.is_cuda and users.is_cuda):
        raise RuntimeError("fold_in_items needs the tables and the audiences on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != dev for t in (P, item_bias, indptr, users, seen_indptr, seen_indices, init,
                                                       init_bias, neg, train_users, train_items)):
        raise RuntimeError("fold_in_items needs every tensor on the device of Q")
    if seen_indices is not None and seen_indices.numel() == 0:
        seen_indptr = seen_indices = None  # (an empty tensor has no address: nothing is seen either way)
    lib = native.load()
    Q_new = _initial_rows(init, init_std, seed, m, d, dev)
    bias_new = None
    if item_bias is not None:
        bias_new = (init_bias.detach().clone().contiguous() if init_bias is not None
                    else torch.zeros(m, dtype=torch.float32, device=dev))
    neg, used = _neg_buffers(neg, epochs, nnz, return_neg, dev)
    roles = torch.full((epochs * m * R,), -1, dtype=torch.int32, device=dev) if return_roles else None
    order = balance_order(indptr[1:] - indptr[:-1]) if balance and m and (nnz or R) else None
    if m and R:
        if users.numel() == 0:
            users = torch.zeros(1, dtype=torch.int32, device=dev)  # (no audiences: an address that is never read)
        with torch.cuda.device(dev):
            native.check(lib.bpr_fold_in_item_rows_roles(
                P.data_ptr(), U, Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d,
                None if seen_indptr is None else seen_indptr.data_ptr(),
                None if seen_indices is None else seen_indices.data_ptr(), indptr.data_ptr(), users.data_ptr(), m,
                None if order is None else order.data_ptr(), epochs, float(lr), float(reg_item),
                native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM, None if neg is None else neg.data_ptr(),
                None if (neg is not None or used is None) else used.data_ptr(), int(seed), int(offset),
                train_users.data_ptr(), train_items.data_ptr(), train_users.numel(), R,
                None if roles is None else roles.data_ptr(), Q_new.data_ptr(),
                None if bias_new is None else bias_new.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    elif m and nnz:
        with torch.cuda.device(dev):
            native.check(lib.bpr_fold_in_item_rows(
                P.data_ptr(), U, Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d,
                None if seen_indptr is None else seen_indptr.data_ptr(),
                None if seen_indices is None else seen_indices.data_ptr(), indptr.data_ptr(), users.data_ptr(), m,
                None if order is None else order.data_ptr(), epochs, float(lr), float(reg_item),
                native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM, None if neg is None else neg.data_ptr(),
                None if (neg is not None or used is None) else used.data_ptr(), int(seed), int(offset),
                Q_new.data_ptr(), None if bias_new is None else bias_new.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream))
    out = ((Q_new,) + ((bias_new,) if bias_new is not None else ()) + ((used,) if return_neg else ())
           + ((roles,) if return_roles else ()))
    return out if len(out) > 1 else Q_new


def _roles(neg_role, train_users, train_items, I: int):
    """(R, train_users, train_items) of a `fold_in_items` call: `neg_role` resolved to the count of negative-role
    steps per row and epoch, the training arrays checked and flattened (None, None when R = 0)."""
    if isinstance(neg_role, str):
        if neg_role != "auto":
            raise ValueError('neg_role must be an int or "auto"')
    elif isinstance(neg_role, bool) or not isinstance(neg_role, int):
        raise ValueError('neg_role must be an int or "auto"')
    elif neg_role < 0:
        raise ValueError("neg_role must be at least 0")
    elif neg_role == 0:
        return 0, None, None
    if train_users is None or train_items is None:
        raise ValueError("neg_role needs train_users and train_items: the training interactions")
    if train_users.dtype != torch.int32 or train_items.dtype != torch.int32:
        raise ValueError("train_users and train_items must be int32")
    train_users, train_items = train_users.reshape(-1).contiguous(), train_items.reshape(-1).contiguous()
    T = train_users.numel()
    if train_items.numel() != T:
        raise ValueError("train_users and train_items must have the same length")
    if T < 1 or T >= 2 ** 31:
        raise ValueError("neg_role needs between 1 and 2^31 - 1 training interactions")
    R = max(1, round(T / max(I - 1, 1))) if neg_role == "auto" else int(neg_role)
    if R >= 2 ** 31:
        raise ValueError("neg_role must be below 2^31")
    return R, train_users, train_items
