"""What the serving wrappers have in common (recommend, retrieve, sample, ranks, rerank, similar, diversify; fold-in
takes `_table` and `seen_csr`), each block once: the table checks, the seen-CSR check, the id normalisation, the
device refusals, the `None`-or-address idiom, the sizing calls, the workspace of a sliced call, the `_rows` /
`_rows_filtered` call of the families that take an item filter, and the one body of recommend and retrieve.

A helper imposes no order: every wrapper calls them in ITS order, and where two wrappers word or condition a check
differently the difference is a parameter — which refusal a malformed call meets, and in which words, is the
wrapper's own (tests/test_serving_refusals_cpu.py, tests/test_gpu_serving_refusals.py; DESIGN.md lists the
differences)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr.item_filter import check_item_filter, check_item_filter_early


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


def call_rows(family: str, device, before: tuple, item_filter: Optional[torch.Tensor], after: tuple) -> None:
    """`bpr_<family>_rows(*before, *after, stream)` on the current stream of `device`; with a filter
    `bpr_<family>_rows_filtered(*before, filter, *after, stream)` — the filter's place in the argument list is where
    the wrapper cuts its own.  No filter goes to the unfiltered entry point, whose messages carry its name."""
    lib = native.load()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if item_filter is None:
            native.check(getattr(lib, f"bpr_{family}_rows")(*before, *after, stream))
        else:
            native.check(getattr(lib, f"bpr_{family}_rows_filtered")(*before, item_filter.data_ptr(), *after, stream))


def best_items(family: str, name: str, k_max: int, P, Q, item_bias, users, k, seen_indptr, seen_indices, *,
               item_slices: int, check_users: bool, item_filter):
    """The body of `recommend` (family "topk") and `retrieve` ("retrieve"): `name` is the caller in the messages,
    `k_max` its largest k.  Their docstrings say what it returns."""
    k = int(k)
    if k > k_max:
        raise ValueError(f"k = {k}: {name} returns at most {k_max} items per user")
    if k < 1:
        raise ValueError("k must be at least 1")
    item_filter = check_item_filter_early(item_filter, Q)
    need_rocm(name, "the tables and the user list", (P, Q, users, item_bias, item_filter),
              (P, Q, item_bias, users, seen_indptr, seen_indices, item_filter), "P")
    native.load()
    P, Q, item_bias, U, I, d = tables(P, Q, item_bias)
    item_filter = check_item_filter(item_filter, I)
    dev = P.device
    users = int32_ids(users, strict=False)
    n = users.numel()
    seen_indptr, seen_indices = seen_csr(seen_indptr, seen_indices, U)
    if check_users and n and bool(((users < 0) | (users >= U)).any()):
        raise ValueError("user id out of range")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    item_slices, ws, ws_bytes = sliced_workspace(family, (n, I, d, k), item_slices, dev)
    call_rows(family, dev,
              (P.data_ptr(), Q.data_ptr(), ptr(item_bias), I, d, users.data_ptr(), n, ptr(seen_indptr),
               ptr(seen_indices)), item_filter,
              (k, item_slices, ptr(ws), ws_bytes, items.data_ptr(), scores.data_ptr()))
    return items, scores
