"""Fold new users into a trained model on the HIP engine: learn p_u from a new user's history against
the FROZEN item table (`bpr_fold_in_rows`, csrc/bpr_foldin.hip).  The result is a [n, d] user table for
`recommend`, `evaluate_topk` and `evaluate_fused`, which take any such table plus a seen CSR.

The reference has no such step (its held-out users' histories are part of the training file,
full-train-with-fold-in.jsonl), so its configs/RQ3/user-split protocol has no BPR entry.

There is no CPU path: tensors must live on a ROCm device.
"""
from __future__ import annotations

from typing import Optional

import torch

from revisit_bpr import native


def balance_order(lengths: torch.Tensor) -> torch.Tensor:
    """The order in which a fold-in launch hands out its rows: longest first (a stable descending
    argsort of the row lengths, int32), so that the rows that take longest start first."""
    return torch.argsort(lengths.reshape(-1), descending=True, stable=True).to(torch.int32)


def _table(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    return t.detach().contiguous()


@torch.no_grad()
def fold_in(Q: torch.Tensor, item_bias: Optional[torch.Tensor], indptr: torch.Tensor, items: torch.Tensor, *,
            epochs: int, lr: float, reg_user: float = 0.0, init: Optional[torch.Tensor] = None,
            init_std: float = 0.0, seed: int = 0, offset: int = 0, neg: Optional[torch.Tensor] = None,
            return_neg: bool = False, balance: bool = True):
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
    """
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError("epochs must be at least 1")
    Q, item_bias = _table(Q, "Q"), _table(item_bias, "item_bias")
    if Q.dim() != 2:
        raise ValueError("Q must be [I, d]")
    I, d = Q.shape
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    if indptr.dtype != torch.int64 or items.dtype != torch.int32:
        raise ValueError("indptr must be int64 and items int32")
    if indptr.dim() != 1 or indptr.numel() < 1:
        raise ValueError("indptr must have n+1 entries")
    indptr, items = indptr.contiguous(), items.reshape(-1).contiguous()
    n = indptr.numel() - 1
    dev = Q.device
    first, last = (int(v) for v in indptr[[0, n]].tolist())
    nnz = last - first
    if first < 0 or nnz < 0 or last > items.numel():
        raise ValueError("indptr does not describe rows of `items`")
    if init is not None and (init.dtype != torch.float32 or tuple(init.shape) != (n, d)):
        raise ValueError("init must be float32 [n, d]")
    if neg is not None:
        if neg.dtype != torch.int32:
            raise ValueError("neg must be int32")
        if neg.numel() != epochs * nnz:
            raise ValueError(f"neg must have epochs * nnz = {epochs * nnz} entries")
    # (the shapes are checked on any device; the work is not done on any)
    if not (Q.is_cuda and indptr.is_cuda and items.is_cuda):
        raise RuntimeError("fold_in needs the item table and the histories on a ROCm device; there is no "
                           "CPU path in libbprcore")
    if any(t is not None and t.device != Q.device for t in (item_bias, indptr, items, init, neg)):
        raise RuntimeError("fold_in needs every tensor on the device of Q")
    lib = native.load()
    if init is not None:
        P_new = init.detach().clone().contiguous()
    elif init_std:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        P_new = torch.randn((n, d), generator=gen, device=dev, dtype=torch.float32) * float(init_std)
    else:
        P_new = torch.zeros((n, d), dtype=torch.float32, device=dev)
    if neg is not None:
        neg = neg.reshape(-1).contiguous()
        used = neg
    else:
        used = torch.zeros(epochs * nnz, dtype=torch.int32, device=dev) if return_neg else None
    if n and nnz:
        order = balance_order(indptr[1:] - indptr[:-1]) if balance else None
        with torch.cuda.device(dev):
            native.check(lib.bpr_fold_in_rows(
                Q.data_ptr(), None if item_bias is None else item_bias.data_ptr(), I, d, indptr.data_ptr(),
                items.data_ptr(), n, None if order is None else order.data_ptr(), epochs, float(lr),
                float(reg_user), native.NEG_GIVEN if neg is not None else native.NEG_UNIFORM,
                None if neg is None else neg.data_ptr(),
                None if (neg is not None or used is None) else used.data_ptr(), int(seed), int(offset),
                P_new.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return (P_new, used) if return_neg else P_new
