"""What the serving wrappers have in common (recommend, retrieve, sample, ranks, rerank, similar, diversify; fold-in
takes `_table` and `seen_csr`), each block once: the table checks, the seen-CSR check, the id normalisation, the
device refusals, the `None`-or-address idiom, the sizing calls and the workspace of a sliced call.

A helper imposes no order: every wrapper calls them in ITS order, and where two wrappers word or condition a check
differently the difference is a parameter — which refusal a malformed call meets, and in which words, is the
wrapper's own (tests/test_serving_refusals_cpu.py, tests/test_gpu_serving_refusals.py; DESIGN.md lists the
differences)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native


def _table(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    return t.detach().contiguous()


def tables(P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor]):
    """(P, Q, item_bias, U, I, d) of float32 tables that fit each other."""
    P, Q, item_bias = _table(P, "P"), _table(Q, "Q"), _table(item_bias, "item_bias")
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError("P [U, d] and Q [I, d] must share the embedding dim")
    (U, d), I = P.shape, Q.shape[0]
    if item_bias is not None and item_bias.numel() != I:
        raise ValueError("item_bias must have one entry per item row")
    return P, Q, item_bias, U, I, d


def seen_csr(seen_indptr: Optional[torch.Tensor], seen_indices: Optional[torch.Tensor], U: int, *,
             together: str = "seen_indptr and seen_indices go together", flat: bool = False):
    """The seen CSR of U users (both None: none), contiguous.  `together`: the words for half a CSR; `flat`
    (fold_in_items): `seen_indptr` must be 1-D as well, and `seen_indices` of any shape is taken as its flat list."""
    if (seen_indptr is None) != (seen_indices is None):
        raise ValueError(together)
    if seen_indptr is None:
        return None, None
    if seen_indptr.dtype != torch.int64 or seen_indices.dtype != torch.int32:
        raise ValueError("seen_indptr must be int64 and seen_indices int32")
    if (flat and seen_indptr.dim() != 1) or seen_indptr.numel() != U + 1:
        raise ValueError("seen_indptr must have U+1 entries")
    return seen_indptr.contiguous(), (seen_indices.reshape(-1) if flat else seen_indices).contiguous()


def int32_ids(t: torch.Tensor, *, strict: bool, name: str = "users") -> torch.Tensor:
    """An id list as flat contiguous int32.  strict: only int32 and int64 are taken; else any dtype is converted."""
    if strict and t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64")
    return t.reshape(-1).to(torch.int32).contiguous()


def need_rocm(name: str, what: str, present, all_tensors, anchor_name: str) -> None:
    """The two device refusals of wrapper `name`: every tensor of `present` on a ROCm device (`what` names them), and
    every tensor of `all_tensors` on the device of the first, which the message calls `anchor_name`.  None: not
    given."""
    if not all(t.is_cuda for t in present if t is not None):
        raise RuntimeError(f"{name} needs {what} on a ROCm device; there is no CPU path in libbprcore")
    anchor = all_tensors[0]
    if any(t is not None and t.device != anchor.device for t in all_tensors[1:]):
        raise RuntimeError(f"{name} needs every tensor on the device of {anchor_name}")


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def query(fn: str, *args, ctype=ctypes.c_int32):
    """An entry point that answers through out-pointers behind its arguments (`_workspace`, `_slices`, `_layout`):
    the value as a Python int, or for a tuple of ctypes the tuple of values."""
    kinds = ctype if isinstance(ctype, tuple) else (ctype,)
    out = [kind() for kind in kinds]
    native.check(getattr(native.load(), fn)(*args, *(ctypes.byref(o) for o in out)))
    return tuple(int(o.value) for o in out) if isinstance(ctype, tuple) else int(out[0].value)


def sliced_workspace(family: str, shape: tuple, item_slices: int, device, *, pre: tuple = (), post: tuple = (),
                     words: bool = False):
    """The slice count a sliced call of `shape` runs with and the workspace of that very count: (item_slices,
    workspace or None, its bytes).  `bpr_<family>_workspace` takes (*shape, *pre, item_slices, *post).  words: the
    workspace is allocated as int64 words instead of bytes."""
    item_slices = query(f"bpr_{family}_slices", *shape, item_slices)
    ws_bytes = query(f"bpr_{family}_workspace", *shape, *pre, item_slices, *post, ctype=ctypes.c_int64)
    if not ws_bytes:
        return item_slices, None, 0
    if words:
        return item_slices, torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=device), ws_bytes
    return item_slices, torch.empty(ws_bytes, dtype=torch.uint8, device=device), ws_bytes
