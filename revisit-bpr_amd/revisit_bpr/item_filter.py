"""The item filter of `recommend`, `retrieve`, `sample_items`, `rank_items` / `evaluate_ranked` and `neighbors` /
`similar_items` / `similar_users` (`item_filter=`): a bitmap over the catalogue that
says which items a call may return — in stock, of a category, licensed, not on a block list.  The kernels take it as
one more eligibility rule beside "not item 0" and "not seen" (csrc/bpr_item_filter.h states the layout once), so a
filtered call returns k items where filtering after the cut returns fewer, and `sample_items`' log_z normalises over
the eligible items only.

Layout: int32 words, bit `i & 31` of word `i >> 5` set = item i is eligible; `4 * ceil(I / 128)` words (whole item
tiles), bits at or past I zero.  Item 0 is never returned whatever its bit says.  `pack_item_filter` builds one,
`unpack_item_filter` reads one back; the wrappers take a packed tensor only, so that a filter is packed once and used
by many calls.
"""
from __future__ import annotations

from typing import Optional

import torch

TILE_ITEMS = 128                  # TOPK_TI: items of a tile
TILE_WORDS = TILE_ITEMS // 32     # FILTER_TILE_WORDS
ALIGN = 16                        # FILTER_ALIGN: bytes


def filter_words(num_items: int) -> int:
    """words of a filter over `num_items` items"""
    return TILE_WORDS * ((int(num_items) + TILE_ITEMS - 1) // TILE_ITEMS)


def _ids(ids, num_items: int, name: str, device) -> torch.Tensor:
    ids = torch.as_tensor(ids, device=device)
    if ids.numel() == 0:  # (an empty list has no integer dtype of its own)
        return torch.zeros(0, dtype=torch.int64, device=device)
    if ids.dtype == torch.bool or ids.is_floating_point() or ids.is_complex():
        raise ValueError(f"{name} must hold integer item ids")
    ids = ids.reshape(-1).to(torch.int64)
    if ids.numel() and bool(((ids < 0) | (ids >= num_items)).any()):
        raise ValueError(f"{name}: item id out of range [0, {num_items})")
    return ids


def pack_item_filter(num_items: int, allow=None, deny=None, mask=None, device=None, first: int = 0) -> torch.Tensor:
    """The packed filter (int32 [4 * ceil(I / 128)]) of exactly one of: `allow`, the eligible ids; `deny`, the ids
    that are not (everything else is); `mask`, bool [I], True = eligible.  Ids are range-checked against
    [0, num_items) and may repeat.  `device`: where the result lives (default: where `mask` / the ids live, else the
    CPU).  `first`: ids below `first` are cleared.  The default stores every bit as given, item 0's too: the kernels
    over an item table never read it as an item, and a filter over the USERS (`similar_users`, `neighbors(first=0)`)
    keeps user 0, who is a user.  `first=1` clears item 0's bit in the stored words as well."""
    num_items = int(num_items)
    if num_items < 1:
        raise ValueError("num_items must be at least 1")
    first = int(first)
    if first < 0:
        raise ValueError("first must be at least 0")
    if sum(x is not None for x in (allow, deny, mask)) != 1:
        raise ValueError("give exactly one of allow, deny and mask")
    given = allow if allow is not None else deny if deny is not None else mask
    if device is None:
        device = given.device if isinstance(given, torch.Tensor) else torch.device("cpu")
    device = torch.device(device)
    if mask is not None:
        m = torch.as_tensor(mask, device=device)
        if m.dtype != torch.bool or m.dim() != 1 or m.numel() != num_items:
            raise ValueError("mask must be bool [num_items]")
        m = m.clone()
    elif allow is not None:
        m = torch.zeros(num_items, dtype=torch.bool, device=device)
        m[_ids(allow, num_items, "allow", device)] = True
    else:
        m = torch.ones(num_items, dtype=torch.bool, device=device)
        m[_ids(deny, num_items, "deny", device)] = False
    nw = filter_words(num_items)
    bits = torch.zeros(nw * 32, dtype=torch.int64, device=device)  # (the tail stays zero)
    bits[:num_items] = m
    bits[:min(first, num_items)] = 0
    weights = torch.ones(32, dtype=torch.int64, device=device) << torch.arange(32, dtype=torch.int64, device=device)
    words = (bits.view(nw, 32) * weights).sum(dim=1)               # in [0, 2^32)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)  # the same 32 bits as int32
    return words.to(torch.int32).contiguous()


def unpack_item_filter(item_filter: torch.Tensor, num_items: int) -> torch.Tensor:
    """bool [num_items] of a packed filter: the inverse of `pack_item_filter(mask=...)` (bits as they are stored:
    item 0's too, although no call returns item 0)"""
    check_item_filter(item_filter, int(num_items))
    w = item_filter.to(torch.int64).unsqueeze(1)
    shifts = torch.arange(32, dtype=torch.int64, device=item_filter.device)
    return ((w >> shifts) & 1).reshape(-1)[:int(num_items)].to(torch.bool)


def check_item_filter_early(item_filter: Optional[torch.Tensor], Q) -> Optional[torch.Tensor]:
    """`check_item_filter` before a wrapper's device refusals, so that a malformed filter is a ValueError on any
    device.  A Q that is no [I, d] tensor is `_serving.tables`' to report, in its words, not as a filter of the wrong
    length: the filter then waits for the second call, behind `tables`."""
    if item_filter is None or not isinstance(Q, torch.Tensor) or Q.dim() != 2:
        return item_filter
    return check_item_filter(item_filter, Q.shape[0])


def check_item_filter(item_filter: Optional[torch.Tensor], num_items: int) -> Optional[torch.Tensor]:
    """What a wrapper asks of `item_filter` before the device is touched: None, or the packed tensor itself — int32,
    1-D, contiguous, `filter_words(num_items)` long.  (Its device is the wrapper's `need_rocm` question.)"""
    if item_filter is None:
        return None
    if not isinstance(item_filter, torch.Tensor) or item_filter.dtype != torch.int32:
        raise ValueError("item_filter must be a packed int32 tensor (pack_item_filter)")
    if item_filter.dim() != 1 or item_filter.numel() != filter_words(num_items):
        raise ValueError(f"item_filter must have {filter_words(num_items)} words for {num_items} items "
                         "(pack_item_filter)")
    if not item_filter.is_contiguous():
        raise ValueError("item_filter must be contiguous")
    return item_filter
