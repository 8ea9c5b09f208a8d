"""Torch-facing handle on the HIP BPR engine (libbprcore.so through ``revisit_bpr.native``).

torch is used for device memory and streams only: every tensor handed in stays owned by the
caller, the engine receives ``data_ptr()``s and mutates the embedding tables in place.  All
methods are asynchronous on the current torch stream.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from revisit_bpr import native
from revisit_bpr.native import (MODE_STREAM, MODE_STRICT, NEG_ADAPTIVE, NEG_DYNAMIC, NEG_GIVEN, NEG_UNIFORM, NEG_WARP,
                                OPT_ADAGRAD, OPT_ADAM, OPT_MOMENTUM, OPT_RMSPROP, OPT_SGD)

__all__ = ["Engine", "MaskedStream", "cu_mask", "resolve_reg_alphas", "MODE_STREAM", "MODE_STRICT", "NEG_ADAPTIVE",
           "NEG_DYNAMIC", "NEG_GIVEN", "NEG_UNIFORM", "NEG_WARP", "OPT_ADAGRAD", "OPT_ADAM", "OPT_MOMENTUM", "OPT_RMSPROP", "OPT_SGD"]


def resolve_reg_alphas(reg_alphas: Optional[dict]) -> tuple[float, float, float]:
    """(user, item, neg) after the rules of the reference's Model.regularization
    (revisit_bpr/models/bpr/model.py:74-86): `all` overrides; missing user/item → 0; missing neg →
    item."""
    reg = reg_alphas or {}
    all_reg, user, item, neg = reg.get("all"), reg.get("user"), reg.get("item"), reg.get("neg")
    if all(r is None for r in (all_reg, user, item, neg)):
        return 0.0, 0.0, 0.0
    if all_reg is not None:
        user = item = neg = all_reg
    user = user or 0
    item = item or 0
    neg = neg or item
    return float(user), float(item), float(neg)


def alias_table(weights: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Walker / Vose alias table over weights[1:] (entry 0, the pad item, is ignored): (accept
    float32 [I], alias int32 [I]) for `Engine.bind_item_weights`."""
    import numpy as np

    w = weights.detach().double().cpu().numpy()[1:]
    n = w.shape[0]
    if n < 1 or (w < 0).any() or not w.sum() > 0:
        raise ValueError("item weights must be non-negative with a positive sum")
    p = w * (n / w.sum())
    accept = np.ones(n + 1, np.float32)
    alias = np.arange(n + 1, dtype=np.int32)
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    while small and large:
        s_, l_ = small.pop(), large.pop()
        accept[s_ + 1] = np.float32(p[s_])
        alias[s_ + 1] = l_ + 1
        p[l_] -= 1.0 - p[s_]
        (small if p[l_] < 1.0 else large).append(l_)
    return torch.from_numpy(accept), torch.from_numpy(alias)


def cu_mask(first: int, count: int, total: int = 256) -> list[int]:
    """32-bit words of a CU mask with bits [first, first + count) set.  On MI300-class parts the
    driver deals the mask bits round-robin over the XCDs (bit i -> XCD i % 8), so a contiguous bit
    range takes the same number of CUs from every XCD."""
    if not (0 <= first and 0 < count and first + count <= total):
        raise ValueError("CU range out of bounds")
    words = [0] * ((total + 31) // 32)
    for b in range(first, first + count):
        words[b // 32] |= 1 << (b % 32)
    return words


class MaskedStream:
    """A HIP stream restricted to a set of CUs (hipExtStreamCreateWithCUMask through
    ``bpr_stream_create``); `.torch` is the same stream as a torch.cuda.ExternalStream.  The split
    refresh sorts on one while the STREAM kernel runs on the complementary one."""

    def __init__(self, device: torch.device, mask_words: Optional[list[int]]) -> None:
        self._lib = native.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        out = ctypes.c_void_p()
        if mask_words:
            arr = (ctypes.c_uint32 * len(mask_words))(*mask_words)
            native.check(self._lib.bpr_stream_create(idx, arr, len(mask_words), ctypes.byref(out)))
        else:
            native.check(self._lib.bpr_stream_create(idx, None, 0, ctypes.byref(out)))
        self.ptr = out.value
        self.torch = torch.cuda.ExternalStream(self.ptr, device=torch.device("cuda", idx))

    def close(self) -> None:
        if getattr(self, "ptr", None):
            self._lib.bpr_stream_destroy(ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class Engine:
    """One bpr_ctx bound to a pair of embedding tables resident in HBM."""

    def __init__(self, P: torch.Tensor, Q: torch.Tensor, item_bias: Optional[torch.Tensor] = None,
                 pad_user: Optional[int] = 0, pad_item: Optional[int] = 0) -> None:
        self._lib = native.load()
        if not (P.is_cuda and Q.is_cuda):
            raise RuntimeError("Engine needs the embedding tables on a ROCm device; there is no "
                               "CPU path in libbprcore")
        for name, t in (("P", P), ("Q", Q), ("item_bias", item_bias)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32 tensor")
        if P.shape[1] != Q.shape[1]:
            raise ValueError("user and item tables must share the embedding dim")
        self.device = P.device
        self.P, self.Q, self.item_bias = P, Q, item_bias
        self.U, self.d = P.shape
        self.I = Q.shape[0]
        self._ctx = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        native.check(self._lib.bpr_ctx_create(ctypes.byref(self._ctx), idx, self._stream()))
        native.check(self._lib.bpr_bind_tables(
            self._ctx, P.data_ptr(), self.U, Q.data_ptr(), self.I, self.d, _ptr(item_bias),
            -1 if pad_user is None else int(pad_user), -1 if pad_item is None else int(pad_item)))
        self._keep: dict[str, object] = {}
        self._scalars = torch.zeros(native.SCALARS, dtype=torch.float32, device=self.device)
        self.opt_kind = OPT_SGD
        self.lds_launches = 0
        # test / measurement aids: the environment is read HERE, once per engine, never by the library
        import os

        seen = os.environ.get("BPR_SEEN") or ("csr" if os.environ.get("BPR_NO_BITMAP") else "")
        if seen:
            self.set_tuning("seen", {"csr": 1, "bitmap": 2, "list": 3}[seen])
        if os.environ.get("BPR_VS_DIRECT") in ("0", "1"):
            self.set_tuning("vs_direct", int(os.environ["BPR_VS_DIRECT"]))
        if os.environ.get("BPR_NO_ADAM_CLOSED"):
            self.set_tuning("adam_closed", 0)
        if os.environ.get("BPR_REFRESH_SUB") in ("1", "2", "4"):
            self.set_tuning("refresh_sub", int(os.environ["BPR_REFRESH_SUB"]))
        if os.environ.get("BPR_HOT_LDS"):  # "rows" or "rows,always"
            v = os.environ["BPR_HOT_LDS"].split(",")
            self.set_hot_lds(int(v[0]), len(v) > 1 and v[1] == "1")
        if os.environ.get("BPR_LDS_TAIL"):
            self.set_tuning("lds_tail", int(os.environ["BPR_LDS_TAIL"]))
        if os.environ.get("BPR_LDS_BLOCK"):
            self.set_tuning("lds_block", int(os.environ["BPR_LDS_BLOCK"]))
        if os.environ.get("BPR_HEAVY_T"):
            self.set_heavy_users(int(os.environ["BPR_HEAVY_T"]))

    def set_heavy_users(self, threshold: int, max_bytes: int = 0) -> None:
        """``bpr_set_heavy_users``: users with more than `threshold` seen items (-1: none) get a precomputed seen
        bitmap in HBM, which the bitmap STREAM kernels stage in LDS at a user change; the table takes at most
        `max_bytes` (0: the current cap) — the threshold is doubled until it fits.  Rebuilt by the next sampling
        STREAM launch."""
        native.check(self._lib.bpr_set_heavy_users(self._ctx, int(threshold), int(max_bytes)))

    def heavy_users(self) -> tuple[int, int]:
        """``bpr_heavy_users``: (users with a row in the heavy table, the threshold it ended at) as the last sampling
        STREAM launch used it; (0, requested threshold) before the table is built."""
        n, t = ctypes.c_int64(), ctypes.c_int32()
        native.check(self._lib.bpr_heavy_users(self._ctx, ctypes.byref(n), ctypes.byref(t)))
        return int(n.value), int(t.value)

    def snapshot_partial(self) -> bool:
        """True while the snapshot the samplers read is a partial one (``bpr_adaptive_snapshot_partial``)."""
        v = ctypes.c_int32()
        native.check(self._lib.bpr_adaptive_snapshot_partial(self._ctx, ctypes.byref(v)))
        return bool(v.value)

    def set_tuning(self, key: str, value: int) -> None:
        """``bpr_set_tuning``: "seen" 0 auto | 1 csr | 2 bitmap | 3 list; "vs_direct" -1 auto | 0 | 1;
        "refresh_sub" 0 | 1 | 2 | 4; "partial_snapshot" 0 | 1; "partial_target" 1..1024; "binned_sort" 1 | 0;
        "binned_split" 0 by shape | 1..16 workgroups per column of the split binned sort."""
        native.check(self._lib.bpr_set_tuning(self._ctx, key.encode(), int(value)))
        self.__dict__.setdefault("_tuning", {})[key] = int(value)

    def tuning(self, key: str, default: int = 0) -> int:
        """What `set_tuning(key, ...)` was last given through this engine (`default`: never set)."""
        return self.__dict__.get("_tuning", {}).get(key, default)

    # ---- plumbing ---------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _sync_stream(self) -> None:
        native.check(self._lib.bpr_set_stream(self._ctx, self._stream()))

    def close(self, fold: bool = True) -> None:
        """Destroy the ctx.  fold (an explicit call: the tables are alive): a communicator with its hot tier still
        open is closed first — `bpr_comm_destroy` folds the exchange in flight and this rank's uncut deltas into the
        item table; the garbage collector's call passes False and `bpr_ctx_destroy` then writes nothing."""
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            if fold:
                self._lib.bpr_comm_destroy(self._ctx)
            self._lib.bpr_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close(fold=False)
        except Exception:
            pass

    def _ids(self, t: torch.Tensor, name: str) -> torch.Tensor:
        if not t.is_cuda:
            raise ValueError(f"{name} must live on the GPU")
        t = t.reshape(-1)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)
        return t.contiguous()

    # ---- configuration ----------------------------------------------------------------------
    def bind_seen_csr(self, indptr: torch.Tensor, indices: torch.Tensor) -> None:
        """indptr [U+1] int64, indices [nnz] int32 (sorted per row, no 0, no duplicates)."""
        if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
            raise ValueError("indptr must be int64 and indices int32")
        if indptr.numel() != self.U + 1:
            raise ValueError("indptr must have U+1 entries")
        indptr, indices = indptr.contiguous(), indices.contiguous()
        self._keep["csr"] = (indptr, indices)
        native.check(self._lib.bpr_bind_seen_csr(self._ctx, indptr.data_ptr(), indices.data_ptr()))

    def recommend(self, users: torch.Tensor, k: int, exclude_seen: bool = True, *, item_slices: int = 0,
                  item_filter: Optional[torch.Tensor] = None):
        """The `k` best items of every user of `users` from the bound tables (`bpr_topk_rows`, see
        revisit_bpr/recommend.py): (items [n, k] int32, scores [n, k] float32), sorted by score descending, ties
        by ascending id, padded with -1 / -inf.  Item 0 is never returned; exclude_seen also leaves out the user's
        row of the CSR given to `bind_seen_csr` (none bound: nothing else to leave out).  Rows an Adam / momentum
        / RMSprop optimizer has not replayed yet are scored as they stand: `flush_lazy()` first
        (`Model.recommend` does).  `item_filter`: a packed filter (revisit_bpr/item_filter.py), only its items are
        eligible; `retrieve`, `sample_items` and `recommend_diverse` take it alike."""
        from revisit_bpr.recommend import recommend

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return recommend(self.P, self.Q, self.item_bias, users, k, indptr, indices, item_slices=item_slices,
                         item_filter=item_filter)

    def sample_items(self, users: torch.Tensor, k: int, exclude_seen: bool = True, **kw):
        """`k` items per user drawn without replacement from softmax(score / temperature) over the user's
        eligible items, in draw order, from the bound tables (`bpr_sample_rows`, see revisit_bpr/sample.py, which
        takes the keywords: temperature, seed, draw_ids, return_keys, return_log_z, item_slices, check_users,
        item_filter): (items [n, k] int32, scores [n, k] float32[, keys][, log_z]), padded with -1 / -inf.  Eligibility is
        `recommend`'s.  Rows an optimizer has not replayed yet are scored as they stand: `flush_lazy()` first
        (`Model.sample_items` does)."""
        from revisit_bpr.sample import sample_items

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return sample_items(self.P, self.Q, self.item_bias, users, k, indptr, indices, **kw)

    def retrieve(self, users: torch.Tensor, k: int, exclude_seen: bool = True, *, item_slices: int = 0,
                 item_filter: Optional[torch.Tensor] = None):
        """`recommend` for `k` up to 1,024, the first stage of a two-stage recommender (`bpr_retrieve_rows`, see
        revisit_bpr/retrieve.py): the same scores, exclusions, order and padding, from the kernel that keeps its
        candidates in device memory.  `item_filter`: a packed filter (revisit_bpr/item_filter.py), only its items are
        eligible.  As `recommend`, rows an optimizer has not replayed yet are scored as they stand: `flush_lazy()`
        first (`Model.retrieve` does)."""
        from revisit_bpr.retrieve import retrieve

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return retrieve(self.P, self.Q, self.item_bias, users, k, indptr, indices, item_slices=item_slices,
                        item_filter=item_filter)

    def rank_items(self, users: torch.Tensor, tgt_indptr: torch.Tensor, tgt_items: torch.Tensor,
                   exclude_seen: bool = True, *, item_slices: int = 0,
                   item_filter: Optional[torch.Tensor] = None):
        """(rank, not_below, score) of every target of every row (row r: user `users[r]`, targets
        `tgt_items[tgt_indptr[r]:tgt_indptr[r + 1]]`) among the user's eligible items, from the bound tables
        (`bpr_rank_rows`, see revisit_bpr/ranks.py).  Item 0 is never eligible; exclude_seen also leaves out the
        user's row of the CSR given to `bind_seen_csr`.  Rows an Adam / momentum / RMSprop optimizer has not
        replayed yet are scored as they stand: `flush_lazy()` first (`Model.rank_items` does).  `item_filter`: a
        packed filter (revisit_bpr/item_filter.py), only its items are eligible, a target outside it included."""
        from revisit_bpr.ranks import rank_items

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return rank_items(self.P, self.Q, self.item_bias, users, tgt_indptr, tgt_items, indptr, indices,
                          item_slices=item_slices, item_filter=item_filter)

    def rerank(self, users: torch.Tensor, cand_items: torch.Tensor, k: int,
               cand_indptr: Optional[torch.Tensor] = None, exclude_seen: bool = True, *,
               return_scores: bool = False, layout: int = 0):
        """The `k` best of each row's own candidates from the bound tables (`bpr_rerank_rows`, see
        revisit_bpr/rerank.py): row r is user `users[r]` with `cand_items[cand_indptr[r]:cand_indptr[r + 1]]`, or
        with the whole 1-D `cand_items` when there is no `cand_indptr`.  (items [n, k] int32, scores [n, k]
        float32), sorted by score descending, ties by ascending id, padded with -1 / -inf; `return_scores` adds
        every candidate's score (-inf: not eligible).  Ids outside 1 .. I-1 are never eligible; exclude_seen also
        leaves out the user's row of the CSR given to `bind_seen_csr`.  Rows an Adam / momentum / RMSprop
        optimizer has not replayed yet are scored as they stand: `flush_lazy()` first (`Model.rerank` does)."""
        from revisit_bpr.rerank import rerank

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return rerank(self.P, self.Q, self.item_bias, users, cand_items, k, cand_indptr, indptr, indices,
                      return_scores=return_scores, layout=layout)

    def score_candidates(self, users: torch.Tensor, cand_items: torch.Tensor,
                         cand_indptr: Optional[torch.Tensor] = None, exclude_seen: bool = True, *, layout: int = 0):
        """The score of every candidate of every row (`rerank` with k = 0): float32 aligned with `cand_items`
        ([n, C] for a shared 1-D list), -inf for a candidate that is not eligible."""
        from revisit_bpr.rerank import score_candidates

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return score_candidates(self.P, self.Q, self.item_bias, users, cand_items, cand_indptr, indptr, indices,
                                layout=layout)

    def similar_items(self, items: torch.Tensor, k: int, metric: str = "cosine", *, item_slices: int = 0,
                      item_filter: Optional[torch.Tensor] = None):
        """The `k` items most similar to each item of `items` by the rows of the bound item table
        (`bpr_neighbors_rows`, see revisit_bpr/similar.py): (ids [n, k] int32, scores [n, k] float32), sorted by
        score descending, ties by ascending id, padded with -1 / -inf; never the item itself, never item 0.
        `metric`: "cosine" or "dot".  The item bias plays no part.  Rows an Adam / momentum / RMSprop optimizer
        has not replayed yet are compared as they stand: `flush_lazy()` first (`Model.similar_items` does).  A
        freshly folded-in row is not in the table: `similar.neighbors(Q_new, engine.Q, torch.arange(m), k,
        first=1)`.  `item_filter`: a packed filter over the items (revisit_bpr/item_filter.py), only its items
        are returned."""
        from revisit_bpr.similar import similar_items

        return similar_items(self.Q, items, k, metric, item_slices=item_slices, item_filter=item_filter)

    def similar_users(self, users: torch.Tensor, k: int, metric: str = "cosine", *, item_slices: int = 0,
                      item_filter: Optional[torch.Tensor] = None):
        """The `k` users most similar to each user of `users` by the rows of the bound user table: as
        `similar_items`, except that user 0 is a user like any other.  A freshly folded-in row:
        `similar.neighbors(P_new, engine.P, torch.arange(m), k)`.  `item_filter`: a packed filter over the USERS
        (`pack_item_filter(U, ...)`; user 0's bit counts), only its users are returned."""
        from revisit_bpr.similar import similar_users

        return similar_users(self.P, users, k, metric, item_slices=item_slices, item_filter=item_filter)

    def diversify(self, cand_items: torch.Tensor, cand_scores: torch.Tensor, k: int, *, lam: float = 0.7,
                  metric: str = "cosine", scale: str = "none", return_mmr: bool = False, layout: int = 0):
        """Greedy MMR over each row's pool of candidates by the rows of the bound item table
        (`bpr_diversify_rows`, see revisit_bpr/diversify.py): `cand_items` / `cand_scores` [n, C] as `recommend` /
        `rerank` return them, C <= 128; (items [n, k] int32, scores [n, k] float32) in pick order, padded with
        -1 / -inf; `return_mmr` adds the objective each pick won with.  Rows an Adam / momentum / RMSprop optimizer
        has not replayed yet are compared as they stand: `flush_lazy()` first (`Model.diversify` does)."""
        from revisit_bpr.diversify import diversify

        return diversify(self.Q, cand_items, cand_scores, k, lam=lam, metric=metric, scale=scale,
                         return_mmr=return_mmr, layout=layout)

    def recommend_diverse(self, users: torch.Tensor, k: int, *, pool: int = 100, lam: float = 0.7,
                          metric: str = "cosine", scale: str = "minmax", exclude_seen: bool = True,
                          item_filter: Optional[torch.Tensor] = None):
        """`recommend(pool)` followed by `diversify(k)` on the bound tables (revisit_bpr/diversify.py): the `k`
        picks of greedy MMR from every user's `pool` best items.  lam = 1 is `recommend(k)` bit for bit.
        `item_filter` is `recommend`'s: the pool holds eligible items only."""
        from revisit_bpr.diversify import recommend_diverse

        indptr, indices = self._keep.get("csr", (None, None)) if exclude_seen else (None, None)
        return recommend_diverse(self.P, self.Q, self.item_bias, users, k, pool=pool, lam=lam, metric=metric,
                                 scale=scale, seen_indptr=indptr, seen_indices=indices, item_filter=item_filter)

    def fold_in(self, indptr: torch.Tensor, items: torch.Tensor, *, epochs: int, lr: Optional[float] = None,
                sampler: str = "uniform", refresh: bool = True, **kwargs) -> torch.Tensor:
        """User rows for NEW users (the rows of the CSR `indptr` / `items`) learnt against the engine's item
        table and bias, which are not changed (`bpr_fold_in_rows`, see revisit_bpr/foldin.py for the keywords).
        `reg_user` defaults to the alpha_user of `set_reg`, `lr` to the learning rate of `set_optimizer`.  The
        item table is made whole first: the hot block an asynchronous cut left is folded and rows a lazy
        optimizer has not replayed yet are flushed.

        `sampler="adaptive"` (`bpr_fold_in_rows_adaptive`; `adaptive_p` as in foldin.fold_in) draws from the
        engine's own snapshot buffers, without a copy.  `refresh=True` runs `adaptive_refresh()` first, after the
        fold and the flush, so the snapshot is the item table's as it stands — and it REPLACES the snapshot the
        training samplers read: a training loop that folds users in mid-epoch should pass `refresh=False`, or
        refresh on its own schedule.  `refresh=False` needs an existing snapshot, and the caller vouches for its
        age: the kernel cannot tell a stale order from a fresh one.

        `sampler="dynamic"` (`candidates`) and `sampler="warp"` (`max_sampled`, `margin`) fold in with the sampler
        the table was trained with (`bpr_fold_in_rows_scored`); the keywords go through to foldin.fold_in as they
        are — the values given to `set_dynamic` / `set_warp` are the training launches' and are not read here.  No
        snapshot is involved, and `refresh` is ignored."""
        from revisit_bpr import foldin

        self._refuse_foldin_adagrad("fold_in", "revisit_bpr.foldin.fold_in")
        if lr is None:
            lr = getattr(self, "_lr", None)
            if lr is None:
                raise ValueError("fold_in needs `lr`: no optimizer was set on this engine")
        kwargs.setdefault("reg_user", getattr(self, "_reg", (0.0, 0.0, 0.0))[0])
        self.hot_fold()
        self.flush_items()
        if sampler == "adaptive":
            if "snapshot" in kwargs:
                raise ValueError("Engine.fold_in draws from the engine's own snapshot")
            if refresh:
                self.adaptive_refresh()
            elif not self._has_snapshot():
                raise RuntimeError("fold_in(sampler='adaptive', refresh=False) needs a snapshot: call "
                                   "adaptive_refresh() first")
            order, sigma = self._snapshot_views(back=False)
            kwargs["snapshot"] = (foldin._PaddedOrder(order), sigma)  # (the engine's buffer carries the slack)
        return foldin.fold_in(self.Q, self.item_bias, indptr, items, epochs=epochs, lr=lr, sampler=sampler, **kwargs)

    def fold_in_items(self, indptr: torch.Tensor, users: torch.Tensor, *, epochs: int, lr: Optional[float] = None,
                      exclude_seen: bool = True, **kwargs):
        """Item rows (and biases, when the engine has an item bias) for NEW items (the rows of the CSR `indptr` /
        `users`: who interacted with each) learnt against the engine's user table, item table and bias, none of
        which is changed (`bpr_fold_in_item_rows`, see revisit_bpr/foldin_items.py for the keywords and the
        return value).  The rows are returned, not appended: `torch.cat((engine.Q, Q_new))` and
        `torch.cat((engine.item_bias, bias_new))` go straight into `recommend`, `rank_items` and `evaluate_*`.
        `reg_item` defaults to the item alpha of `set_reg`, `lr` to the learning rate of `set_optimizer`.
        `exclude_seen`: sampled negatives are unseen by the triple's user according to the CSR given to
        `bind_seen_csr` (False, or none bound: any item but 0).  `neg_role`, `train_users`, `train_items` and
        `return_roles` (the item's second role, as the negative of training interactions outside its audience) go
        through unchanged.  Both tables are made whole first: the hot block an
        asynchronous cut left is folded and rows a lazy optimizer has not replayed yet are flushed."""
        from revisit_bpr import foldin_items

        self._refuse_foldin_adagrad("fold_in_items", "revisit_bpr.foldin_items.fold_in_items")
        if lr is None:
            lr = getattr(self, "_lr", None)
            if lr is None:
                raise ValueError("fold_in_items needs `lr`: no optimizer was set on this engine")
        kwargs.setdefault("reg_item", getattr(self, "_reg", (0.0, 0.0, 0.0))[1])
        if "seen_indptr" in kwargs or "seen_indices" in kwargs:
            raise ValueError("Engine.fold_in_items draws against the engine's own seen CSR")
        if exclude_seen:
            kwargs["seen_indptr"], kwargs["seen_indices"] = self._keep.get("csr", (None, None))
        self.hot_fold()
        self.flush_items()
        self.flush_lazy()
        return foldin_items.fold_in_items(self.P, self.Q, self.item_bias, indptr, users, epochs=epochs, lr=lr,
                                          **kwargs)

    def _refuse_foldin_adagrad(self, who: str, plain: str) -> None:
        """The fold-in kernels take plain sequential SGD steps.  Under the other kinds the engine's rate is an SGD
        rate all the same; Adagrad's multiplies g / sqrt(sum) and means something else, and there is no Adagrad
        fold-in kernel: refused before anything is folded, flushed or launched."""
        if self.opt_kind == OPT_ADAGRAD:
            raise native.BprError(native.ERR_UNSUPPORTED,
                                  f"Engine.{who}: the fold-in kernels are plain SGD and the engine's optimizer is "
                                  f"Adagrad; call {plain} on the tables with an SGD learning rate")

    def _has_snapshot(self) -> bool:
        """True once a refresh has published a snapshot (`adaptive_snapshot()` would succeed)."""
        self._sync_stream()
        return self._lib.bpr_adaptive_get_snapshot(self._ctx, None, None) == native.OK

    def bind_item_weights(self, weights: Optional[torch.Tensor]) -> None:
        """Item weights of the uniform sampler (count_i ** neg_sampling_alpha of the reference's
        BPRExperiment): [I] non-negative; None = uniform."""
        if weights is None:
            self._keep.pop("item_weights", None)
            native.check(self._lib.bpr_bind_item_weights(self._ctx, None, None))
            return
        if weights.numel() != self.I:
            raise ValueError("item weights must have one entry per item row")
        accept, alias = alias_table(weights)
        accept, alias = accept.to(self.device), alias.to(self.device)
        self._keep["item_weights"] = (accept, alias)
        native.check(self._lib.bpr_bind_item_weights(self._ctx, accept.data_ptr(), alias.data_ptr()))

    def set_reg(self, user: float, item: float, neg: float) -> None:
        native.check(self._lib.bpr_set_reg(self._ctx, user, item, neg))
        self._reg = (float(user), float(item), float(neg))

    def set_optimizer(self, kind: int, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                      nesterov: bool = False, betas=(0.9, 0.999), eps: float = 1e-8,
                      alpha: float = 0.99, lr_decay: float = 0.0) -> None:
        """`lr_decay`: torch.optim.Adagrad's (OPT_ADAGRAD only; its `eps` default in torch is 1e-10)."""
        prm = native.OptParams(lr, momentum, dampening, int(nesterov), betas[0], betas[1], eps,
                               alpha, lr_decay)
        native.check(self._lib.bpr_set_optimizer(self._ctx, kind, ctypes.byref(prm)))
        self.opt_kind = kind
        self._momentum = momentum
        self._lr = float(lr)

    def bind_opt_state(self, mP=None, vP=None, mQ=None, vQ=None, mb=None, vb=None) -> None:
        self._keep["opt_state"] = (mP, vP, mQ, vQ, mb, vb)
        native.check(self._lib.bpr_bind_opt_state(self._ctx, _ptr(mP), _ptr(vP), _ptr(mQ), _ptr(vQ),
                                                  _ptr(mb), _ptr(vb)))

    def alloc_opt_state(self) -> dict:
        """Zero state tensors of the shapes the current optimizer kind needs, bound to the ctx (Adagrad: only the
        `v` tensors, its `sum`; fill them for a non-zero initial_accumulator_value)."""
        z = torch.zeros_like
        need_m = self.opt_kind in (OPT_MOMENTUM, OPT_ADAM) or (
            self.opt_kind == OPT_RMSPROP and getattr(self, "_momentum", 0.0) > 0)
        need_v = self.opt_kind in (OPT_ADAM, OPT_RMSPROP, OPT_ADAGRAD)
        st = {
            "mP": z(self.P) if need_m else None, "vP": z(self.P) if need_v else None,
            "mQ": z(self.Q) if need_m else None, "vQ": z(self.Q) if need_v else None,
            "mb": z(self.item_bias) if need_m and self.item_bias is not None else None,
            "vb": z(self.item_bias) if need_v and self.item_bias is not None else None,
        }
        self.bind_opt_state(**st)
        return st

    # ---- negative sampling ------------------------------------------------------------------
    def sample_uniform(self, users: torch.Tensor, seed: int, offset: int = 0) -> torch.Tensor:
        self._sync_stream()
        users = self._ids(users, "users")
        out = torch.empty_like(users)
        native.check(self._lib.bpr_sample_uniform(self._ctx, users.data_ptr(), users.numel(), seed,
                                                  offset, out.data_ptr()))
        return out

    def set_dynamic(self, candidates: int) -> None:
        """Candidates per triple of `train_stream(sampler=NEG_DYNAMIC)` (``bpr_set_dynamic``): 1 .. 32, default 4."""
        native.check(self._lib.bpr_set_dynamic(self._ctx, int(candidates)))

    def sample_dynamic(self, users: torch.Tensor, candidates: int, seed: int, offset: int = 0,
                       return_scores: bool = False):
        """Dynamic negative sampling (``bpr_sample_dynamic``): per entry of `users` the highest-scoring of the first
        `candidates` unseen items of `sample_uniform`'s candidate stream, scored on the tables as they are now.
        candidates = 1 is `sample_uniform`.  return_scores: also the picks' scores, fp32."""
        self._sync_stream()
        users = self._ids(users, "users")
        out = torch.empty_like(users)
        score = torch.empty(users.numel(), dtype=torch.float32, device=self.device) if return_scores else None
        native.check(self._lib.bpr_sample_dynamic(self._ctx, users.data_ptr(), users.numel(), int(candidates), seed,
                                                  offset, out.data_ptr(), _ptr(score)))
        return (out, score) if return_scores else out

    def set_warp(self, max_sampled: int, margin: float = 1.0) -> None:
        """The WARP objective of `train_stream(sampler=NEG_WARP)` (``bpr_set_warp``): at most `max_sampled` (1 .. 32,
        default 10) unseen candidates tried per triple, a violator comes within `margin` (> 0, default 1.0) of the
        positive's score."""
        native.check(self._lib.bpr_set_warp(self._ctx, int(max_sampled), float(margin)))

    def sample_warp(self, users: torch.Tensor, pos: torch.Tensor, max_sampled: int, seed: int, offset: int = 0,
                    margin: float = 1.0, return_scores: bool = False):
        """The WARP draw (``bpr_sample_warp``) on the tables as they are now: per (user, positive) the first of the
        first `max_sampled` unseen items of `sample_uniform`'s candidate stream whose score exceeds the positive's
        less `margin`.  Returns (neg, tries): neg = -1 and tries = 0 where nothing violates (the triple WARP skips);
        return_scores: also (x_pos, x_neg), fp32, x_neg = 0 where skipped."""
        self._sync_stream()
        users, pos = self._ids(users, "users"), self._ids(pos, "pos")
        if users.numel() != pos.numel():
            raise ValueError("sample_warp: users and pos differ in length")
        n = users.numel()
        neg, tries = torch.empty_like(users), torch.empty_like(users)
        xp = torch.empty(n, dtype=torch.float32, device=self.device) if return_scores else None
        xn = torch.empty(n, dtype=torch.float32, device=self.device) if return_scores else None
        native.check(self._lib.bpr_sample_warp(self._ctx, users.data_ptr(), pos.data_ptr(), n, int(max_sampled),
                                               float(margin), seed, offset, neg.data_ptr(), tries.data_ptr(),
                                               _ptr(xp), _ptr(xn)))
        return (neg, tries, xp, xn) if return_scores else (neg, tries)

    def adaptive_refresh(self) -> None:
        """AdaptiveSampler.update_stats: snapshot of the item table as of now, in stream order."""
        self._sync_stream()
        native.check(self._lib.bpr_adaptive_refresh(self._ctx))

    def adaptive_refresh_begin(self) -> None:
        """Split refresh, first half: the snapshot's keys are cut from the item table NOW (stream
        order) and sorted on the side stream while this stream keeps working; the samplers keep
        reading the previous snapshot until `adaptive_refresh_commit`."""
        self._sync_stream()
        native.check(self._lib.bpr_adaptive_refresh_begin(self._ctx))

    def adaptive_refresh_commit(self) -> None:
        """Split refresh, second half: launches after this call read the snapshot cut by the last
        `adaptive_refresh_begin` (this stream waits for the side stream's sort)."""
        self._sync_stream()
        native.check(self._lib.bpr_adaptive_refresh_commit(self._ctx))

    def _snapshot_views(self, back: bool) -> tuple[torch.Tensor, torch.Tensor]:
        """The engine's snapshot buffers as tensors (no copy): order [d, I] int32, sigma [d] fp32."""
        o, g = ctypes.c_void_p(), ctypes.c_void_p()
        native.check(self._lib.bpr_adaptive_snapshot_ptrs(self._ctx, int(back), ctypes.byref(o),
                                                          ctypes.byref(g)))

        class _Dev:  # torch reads device memory it does not own through this protocol
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr,
                                                 "data": (ptr, False), "version": 2}

        order = torch.as_tensor(_Dev(o.value, (self.d, self.I), "<i4"), device=self.device)
        sigma = torch.as_tensor(_Dev(g.value, (self.d,), "<f4"), device=self.device)
        return order, sigma

    def adaptive_refresh_sharded(self, rank: int, world: int, group=None, force: bool = False) -> None:
        """``adaptive_refresh`` with the sort shared by the ranks of a multi-GPU job: this rank
        sorts d / world factors of ITS replica of the item table, an all-gather hands every rank
        every factor's order (10 MB at ML-20M / d = 128) and the same snapshot is published
        everywhere.  Falls back to the full refresh when d does not divide by world.
        force: take the sharded route with ONE rank too (part + all-gather + publish through the process
        group: bench.py --force-dist)."""
        import torch.distributed as dist

        if (world <= 1 and not force) or self.d % max(world, 1) != 0:
            return self.adaptive_refresh()
        self._sync_stream()
        if world <= 1:  # forced: one rank's share is every factor — a full refresh, then the same two
            self.adaptive_refresh()  # all-gathers over the published snapshot (the collective path, one rank)
            order, sigma = self._snapshot_views(back=False)
            dist.all_gather_into_tensor(order.view(-1), order.view(-1).clone(), group=group)
            dist.all_gather_into_tensor(sigma, sigma.clone(), group=group)
            return
        per = self.d // world
        native.check(self._lib.bpr_adaptive_refresh_part(self._ctx, rank * per, (rank + 1) * per))
        order, sigma = self._snapshot_views(back=True)
        mine_o = order[rank * per:(rank + 1) * per].clone()
        mine_s = sigma[rank * per:(rank + 1) * per].clone()
        dist.all_gather_into_tensor(order.view(-1), mine_o.view(-1), group=group)
        dist.all_gather_into_tensor(sigma, mine_s, group=group)
        native.check(self._lib.bpr_adaptive_refresh_publish(self._ctx))

    # ---- multi-GPU inside the library (RCCL behind the C ABI; distributed.ItemSync is the torch twin)
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId through the library: rank 0 calls it and ships the 128 bytes to the others."""
        buf = ctypes.create_string_buffer(128)
        native.check(native.load().bpr_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """Collective: the ctx gets an RCCL communicator; the reconciliation base is cut from the item
        table as it is now (identical on every rank)."""
        self._sync_stream()
        native.check(self._lib.bpr_comm_init(self._ctx, ctypes.c_char_p(unique_id), rank, world))

    def item_sync(self) -> None:
        """Steady-state reconciliation step (fold the all-reduce in flight, cut the next delta,
        all-reduce it on the communicator's stream): `bpr_item_sync`."""
        self._sync_stream()
        native.check(self._lib.bpr_item_sync(self._ctx))

    def item_sync_finish(self) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_item_sync_finish(self._ctx))

    def item_sync_rebase(self) -> None:
        """After the item table was overwritten in place (checkpoint restore): the reconciliation
        bases are cut again from the tables as they are (identical on every rank)."""
        self._sync_stream()
        native.check(self._lib.bpr_item_sync_rebase(self._ctx))

    def comm_hot_tier(self, items: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
        """Two tiers inside the library: the hot set (same list on every rank) whose delta block
        `hot_sync` exchanges after every launch; `item_sync` stays the cold rows' per-period step."""
        import numpy as np

        self._sync_stream()
        it = np.ascontiguousarray(items.detach().cpu().numpy(), dtype=np.int32)
        cn = None if counts is None else np.ascontiguousarray(counts.detach().cpu().numpy(), dtype=np.uint32)
        native.check(self._lib.bpr_comm_hot_tier(
            self._ctx, it.ctypes.data_as(ctypes.c_void_p), int(it.size),
            None if cn is None else cn.ctypes.data_as(ctypes.c_void_p)))

    def hot_sync(self) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_hot_sync(self._ctx))

    def comm_destroy(self) -> None:
        native.check(self._lib.bpr_comm_destroy(self._ctx))

    REFRESH_ROUTES = ("radix", "binned", "binned_split", "partial", "device")

    def refresh_info(self) -> dict:
        """``bpr_adaptive_refresh_info``: what the last completed refresh ran — {"route": one of REFRESH_ROUTES (None
        before the first refresh), "route_id", "g": workgroups per column of the binned sort, "items": keys per
        thread of the kernel instantiation, "sub": workgroups per column of the radix sort or fallback,
        "fallback_columns": columns the split binned sort handed to its fallback (None on the other routes)}.
        A diagnostic: it waits for the stream."""
        self._sync_stream()
        out = (ctypes.c_int32 * native.REFRESH_INFO_LEN)()
        native.check(self._lib.bpr_adaptive_refresh_info(self._ctx, out))
        route, g, items, sub, fell = (int(v) for v in out[:5])
        return {"route": self.REFRESH_ROUTES[route] if route >= 0 else None, "route_id": route, "g": g, "items": items,
                "sub": sub, "fallback_columns": fell if fell >= 0 else None}

    def refresh_pending(self) -> bool:
        out = ctypes.c_int32(0)
        native.check(self._lib.bpr_adaptive_refresh_pending(self._ctx, ctypes.byref(out)))
        return bool(out.value)

    def set_side_stream(self, stream: Optional["MaskedStream"]) -> None:
        """The stream the split refresh sorts on (None: a plain stream owned by the library)."""
        # (the library synchronises the stream it is about to let go of: the old one must still exist then —
        # the reference kept here is replaced AFTER the call)
        native.check(self._lib.bpr_set_side_stream(self._ctx, None if stream is None else stream.ptr))
        self._keep["side_stream"] = stream

    def sample_adaptive(self, users: torch.Tensor, p: float, seed: int, offset: int = 0,
                        return_draws: bool = False):
        self._sync_stream()
        users = self._ids(users, "users")
        neg = torch.empty_like(users)
        fac = torch.empty_like(users) if return_draws else None
        rnk = torch.empty_like(users) if return_draws else None
        native.check(self._lib.bpr_sample_adaptive(self._ctx, users.data_ptr(), users.numel(), p,
                                                   seed, offset, neg.data_ptr(), _ptr(fac),
                                                   _ptr(rnk)))
        return (neg, fac, rnk) if return_draws else neg

    def adaptive_pick(self, users, factor, rank) -> torch.Tensor:
        self._sync_stream()
        users, factor, rank = (self._ids(users, "users"), self._ids(factor, "factor"),
                               self._ids(rank, "rank"))
        neg = torch.empty_like(users)
        native.check(self._lib.bpr_adaptive_pick(self._ctx, users.data_ptr(), factor.data_ptr(),
                                                 rank.data_ptr(), users.numel(), neg.data_ptr()))
        return neg

    def adaptive_snapshot(self) -> tuple[torch.Tensor, torch.Tensor]:
        self._sync_stream()
        order = torch.empty((self.d, self.I), dtype=torch.int32, device=self.device)
        sigma = torch.empty(self.d, dtype=torch.float32, device=self.device)
        native.check(self._lib.bpr_adaptive_get_snapshot(self._ctx, order.data_ptr(),
                                                         sigma.data_ptr()))
        return order, sigma

    def adaptive_sigma(self) -> torch.Tensor:
        """sigma_f of the current snapshot (AdaptiveSampler._factor_std), [d] fp32."""
        self._sync_stream()
        sigma = torch.empty(self.d, dtype=torch.float32, device=self.device)
        native.check(self._lib.bpr_adaptive_get_snapshot(self._ctx, None, sigma.data_ptr()))
        return sigma

    # ---- hot path ---------------------------------------------------------------------------
    def _outs(self, B: int, want_logits: bool, scalars: Optional[torch.Tensor]):
        lp = torch.empty(B, dtype=torch.float32, device=self.device) if want_logits else None
        ln = torch.empty(B, dtype=torch.float32, device=self.device) if want_logits else None
        if scalars is None:
            scalars = torch.zeros(native.SCALARS, dtype=torch.float32, device=self.device)
        return lp, ln, scalars

    def forward(self, users, pos, neg, scalars=None):
        self._sync_stream()
        users, pos, neg = self._ids(users, "users"), self._ids(pos, "pos"), self._ids(neg, "neg")
        lp, ln, sc = self._outs(users.numel(), True, scalars)
        native.check(self._lib.bpr_forward(self._ctx, users.data_ptr(), pos.data_ptr(),
                                           neg.data_ptr(), users.numel(), lp.data_ptr(),
                                           ln.data_ptr(), sc.data_ptr()))
        return lp, ln, sc

    def forward_grad(self, users, pos, neg, scalars=None):
        self._sync_stream()
        users, pos, neg = self._ids(users, "users"), self._ids(pos, "pos"), self._ids(neg, "neg")
        lp, ln, sc = self._outs(users.numel(), True, scalars)
        native.check(self._lib.bpr_forward_grad(self._ctx, users.data_ptr(), pos.data_ptr(),
                                                neg.data_ptr(), users.numel(), lp.data_ptr(),
                                                ln.data_ptr(), sc.data_ptr()))
        return lp, ln, sc

    def apply(self) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_apply(self._ctx))

    def discard_grad(self) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_discard_grad(self._ctx))

    def get_grad(self):
        self._sync_stream()
        gP, gQ = torch.empty_like(self.P), torch.empty_like(self.Q)
        gb = torch.empty(self.I, dtype=torch.float32, device=self.device)
        native.check(self._lib.bpr_get_grad(self._ctx, gP.data_ptr(), gQ.data_ptr(),
                                            gb.data_ptr()))
        return gP, gQ, gb

    def step(self, users, pos, neg=None, mode: int = MODE_STRICT, sampler: int = NEG_GIVEN,
             adaptive_p: float = 0.01, seed: int = 0, offset: int = 0, scalars=None,
             want_logits: bool = True):
        """One reference iteration (sample → forward → backward → optimizer step)."""
        self._sync_stream()
        users, pos = self._ids(users, "users"), self._ids(pos, "pos")
        if neg is None:
            neg = torch.empty_like(users)
        else:
            neg = self._ids(neg, "neg")
        lp, ln, sc = self._outs(users.numel(), want_logits and mode == MODE_STRICT, scalars)
        native.check(self._lib.bpr_step(self._ctx, users.data_ptr(), pos.data_ptr(),
                                        neg.data_ptr(), users.numel(), mode, sampler, adaptive_p,
                                        seed, offset, _ptr(lp), _ptr(ln), sc.data_ptr()))
        return lp, ln, sc, neg

    def train_stream(self, users, pos, sampler: int = NEG_UNIFORM, neg: Optional[torch.Tensor] = None,
                     adaptive_p: float = 0.01, seed: int = 0, offset: int = 0,
                     max_inflight: int = 0, scalars: Optional[torch.Tensor] = None,
                     cut: bool = False) -> None:
        """STREAM mode over users/pos (int32, on device) in one launch; `scalars` (if given) is
        added to.  cut=True: the launch's epilogue also cuts the keys of the next adaptive snapshot
        (``bpr_train_stream_cut``) — the next `adaptive_refresh_begin` only queues the sort.
        cut="async": that cut runs on the side stream beside the NEXT launch and folds nothing
        (``bpr_train_stream_acut``); call `hot_fold()` before reading the item table's storage.
        sampler=NEG_DYNAMIC: the hardest of `set_dynamic`'s candidates per triple; `neg` (if given) receives the picks.
        sampler=NEG_WARP: the WARP objective with `set_warp`'s parameters — the first violator, a step weighted by
        log(estimated rank), no step where nothing violates (`neg` receives -1 there; `scalars` count stepped triples
        only and slot 0 carries sum L (margin - x_i + x_k))."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("train_stream takes int32 id tensors (no hidden copies on the hot path)")
        if sampler == NEG_GIVEN and neg is None:
            raise ValueError("sampler NEG_GIVEN needs `neg`")
        fn = (self._lib.bpr_train_stream_acut if cut == "async" else
              self._lib.bpr_train_stream_cut if cut else self._lib.bpr_train_stream)
        native.check(fn(self._ctx, users.data_ptr(), pos.data_ptr(), _ptr(neg), users.numel(),
                        sampler, adaptive_p, seed, offset, max_inflight, _ptr(scalars)))
        self.lds_launches += self._lib.bpr_stream_lds_rows(self._ctx) > 0  # launches the LDS-tier kernel ran (r6)

    def set_bias_tracking(self, on: bool) -> None:
        """item_bias during STREAM launches (``bpr_set_bias_tracking``): on = a launch skips re-reading the
        dense vector while the library knows its own one-item-per-line table is current.  Only for a
        loop that owns the vector between its launches (fast.StreamTrainer switches it on for the
        duration of one epoch call, bench.py for its run): a write through torch that the library
        cannot see must be declared with `bias_written()`."""
        native.check(self._lib.bpr_set_bias_tracking(self._ctx, int(bool(on))))

    def bias_written(self) -> None:
        native.check(self._lib.bpr_bias_written(self._ctx))

    def train_strict(self, users, pos, batch_size: int, sampler: int = NEG_UNIFORM,
                     neg: Optional[torch.Tensor] = None, adaptive_p: float = 0.01, seed: int = 0,
                     offset: int = 0, refresh_every: int = 0,
                     scalars: Optional[torch.Tensor] = None) -> None:
        """STRICT mini-batch epoch (any optimizer) with the batch loop inside the library."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("train_strict takes int32 id tensors")
        if neg is None:
            if sampler == NEG_GIVEN:
                raise ValueError("sampler NEG_GIVEN needs `neg`")
            neg = torch.empty(max(batch_size, 1), dtype=torch.int32, device=self.device)
        native.check(self._lib.bpr_train_strict(self._ctx, users.data_ptr(), pos.data_ptr(),
                                                neg.data_ptr(), users.numel(), batch_size, sampler,
                                                adaptive_p, seed, offset, refresh_every,
                                                _ptr(scalars)))

    def train_stream_batched(self, users, pos, batch_size: int, sampler: int = NEG_UNIFORM,
                             neg: Optional[torch.Tensor] = None, adaptive_p: float = 0.01,
                             seed: int = 0, offset: int = 0, max_inflight: int = 0,
                             scalars: Optional[torch.Tensor] = None) -> None:
        """BATCHED STREAM over users/pos (int32, on device, shuffled — not grouped by user) in one
        launch, any optimizer: virtual mini-batches of `batch_size` consecutive triples, one
        torch.optim step per row and batch (see include/bprcore.h)."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("train_stream_batched takes int32 id tensors")
        if sampler == NEG_GIVEN and neg is None:
            raise ValueError("sampler NEG_GIVEN needs `neg`")
        native.check(self._lib.bpr_train_stream_batched(
            self._ctx, users.data_ptr(), pos.data_ptr(), _ptr(neg), users.numel(), batch_size,
            sampler, adaptive_p, seed, offset, max_inflight, _ptr(scalars)))

    def train_stream_batched_scored(self, users, pos, batch_size: int, sampler: int,
                                    neg: Optional[torch.Tensor] = None, tries: Optional[torch.Tensor] = None,
                                    seed: int = 0, offset: int = 0, max_inflight: int = 0,
                                    scalars: Optional[torch.Tensor] = None) -> None:
        """`train_stream_batched` with sampler NEG_DYNAMIC or NEG_WARP (``bpr_train_stream_batched_scored``), any
        optimizer: the draw of `sample_dynamic` / `sample_warp` on every row's view as of the previous virtual step,
        with `set_dynamic` / `set_warp`'s values.  neg / tries (int32 [n], optional) receive the picks (-1: a triple
        WARP skips) and WARP's tries (0: skipped; 1 for every dynamic triple).  scalars for NEG_WARP: the WARP loss,
        the L2 term, sum |x_i - x_k| and the count, over the stepped triples."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("train_stream_batched_scored takes int32 id tensors")
        for name, t in (("neg", neg), ("tries", tries)):
            if t is not None and (t.dtype != torch.int32 or t.numel() < users.numel() or not t.is_contiguous()):
                raise ValueError(f"train_stream_batched_scored: {name} must be a contiguous int32 tensor of n entries")
        native.check(self._lib.bpr_train_stream_batched_scored(
            self._ctx, users.data_ptr(), pos.data_ptr(), _ptr(neg), _ptr(tries), users.numel(), batch_size,
            sampler, seed, offset, max_inflight, _ptr(scalars)))

    def shuffle_epoch(self, users: torch.Tensor, pos: torch.Tensor, seed: int,
                      out: Optional[tuple[torch.Tensor, torch.Tensor]] = None):
        """Seeded pseudo-random permutation of the training triples (on device)."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("shuffle_epoch takes int32 id tensors")
        uo, po = out if out is not None else (torch.empty_like(users), torch.empty_like(pos))
        native.check(self._lib.bpr_shuffle_epoch(self._ctx, users.data_ptr(), pos.data_ptr(),
                                                 users.numel(), seed, uo.data_ptr(), po.data_ptr()))
        return uo, po

    def set_stream_opts(self, grouped_by_user: bool, run_len: int = 0) -> None:
        native.check(self._lib.bpr_set_stream_opts(self._ctx, int(grouped_by_user), run_len))

    def stream_run_len(self) -> int:
        """Run length the last STREAM launch used (run_len = 0 lets the library pick it)."""
        return int(self._lib.bpr_stream_run_len(self._ctx))

    def set_hot_lds(self, rows: int, always: bool = False) -> None:
        """``bpr_set_hot_lds``: the `rows` most popular hot rows take a CU's updates in LDS (flushed at the
        workgroup's exit): a hot row is one launch stale across CUs — switch it on by ``fast.lag_within_budget``.
        ``always``: also for launches that do not fill the chip (tests)."""
        native.check(self._lib.bpr_set_hot_lds(self._ctx, int(rows), int(always)))

    def stream_lds_rows(self) -> int:
        """LDS rows of the last STREAM launch (0: the plain kernel ran)."""
        return int(self._lib.bpr_stream_lds_rows(self._ctx))

    def hot_fold(self) -> None:
        """Fold the hot rows' deltas an asynchronous cut left in the block (no-op otherwise): after it
        the item table's storage is whole for a direct reader (eval, checkpoint)."""
        self._sync_stream()
        native.check(self._lib.bpr_hot_fold(self._ctx))

    def set_hot_rows(self, hot_rows: int = 256, replicas: int = 1) -> None:
        """Replica delta rows for the most popular item rows in STREAM mode (0 = off); takes
        effect at the next plan_epoch."""
        native.check(self._lib.bpr_set_hot_rows(self._ctx, hot_rows, replicas))

    # ---- two-tier reconciliation, hot tier (revisit_bpr.distributed.ItemSync drives it)
    def set_hot_items(self, items: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
        """The hot set as given (the ranks of a job agree on it): `items` int32 ids in the canonical
        order of the exchange buffers; `counts` [I] positives per item (steers the placement)."""
        import numpy as np

        it = np.ascontiguousarray(items.detach().cpu().numpy(), dtype=np.int32)
        cn = None if counts is None else np.ascontiguousarray(counts.detach().cpu().numpy(), dtype=np.uint32)
        native.check(self._lib.bpr_set_hot_items(
            self._ctx, it.ctypes.data_as(ctypes.c_void_p), int(it.size),
            None if cn is None else cn.ctypes.data_as(ctypes.c_void_p)))

    def hot_rows(self) -> int:
        v = ctypes.c_int32()
        native.check(self._lib.bpr_hot_rows(self._ctx, ctypes.byref(v)))
        return v.value

    def hot_tier_begin(self, hot_base: torch.Tensor) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_hot_tier_begin(self._ctx, hot_base.data_ptr()))

    def hot_exchange(self, hot_base: torch.Tensor, tot: torch.Tensor, fold_prev: bool, cut: bool,
                     cold_base: Optional[torch.Tensor] = None) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_hot_exchange(self._ctx, hot_base.data_ptr(), tot.data_ptr(),
                                                int(fold_prev), int(cut), _ptr(cold_base)))

    def sync_cut(self, hot_base, hot_tot, hot_fold_prev: bool, cold_base, cold_own, cold_tot, scale: float,
                 cold_mode: int) -> None:
        """`bpr_sync_cut`: hot-tier step + cold-tier step + the cut of the next snapshot's keys in one
        pass over the item table (after a `train_stream(cut=True)` under the hot tier)."""
        self._sync_stream()
        native.check(self._lib.bpr_sync_cut(self._ctx, _ptr(hot_base), _ptr(hot_tot), int(hot_fold_prev),
                                            _ptr(cold_base), _ptr(cold_own), _ptr(cold_tot), scale, cold_mode))

    def hot_tier_end(self) -> None:
        native.check(self._lib.bpr_hot_tier_end(self._ctx))

    def plan_epoch(self, users: torch.Tensor, pos: torch.Tensor, chunk: int, seed: int,
                   out: Optional[tuple[torch.Tensor, torch.Tensor]] = None, sorted_input: bool = False):
        """Shuffle the training triples into chunks of `chunk`, each grouped by user (on device).
        sorted_input: a PROMISE that `users` is sorted by user id (`users_sorted` checks it once per training
        set): the same plan in one radix pass instead of three (bpr_set_tuning "plan_input_sorted")."""
        self._sync_stream()
        if users.dtype != torch.int32 or pos.dtype != torch.int32:
            raise ValueError("plan_epoch takes int32 id tensors")
        if bool(sorted_input) != getattr(self, "_plan_sorted", False):
            self._plan_sorted = bool(sorted_input)
            self.set_tuning("plan_input_sorted", int(self._plan_sorted))
        uo, po = out if out is not None else (torch.empty_like(users), torch.empty_like(pos))
        native.check(self._lib.bpr_plan_epoch(self._ctx, users.data_ptr(), pos.data_ptr(),
                                              users.numel(), chunk, seed, uo.data_ptr(),
                                              po.data_ptr()))
        return uo, po

    @staticmethod
    def users_sorted(users: torch.Tensor) -> bool:
        """Is the triple list in CSR order (sorted by user)?  One pass + one host read: call it once per training set."""
        return bool(users.numel() < 2 or (users[1:] >= users[:-1]).all().item())

    def plan_chunk(self, users: torch.Tensor, pos: torch.Tensor, chunk: int, seed: int, index: int,
                   out: tuple[torch.Tensor, torch.Tensor], on_side: bool = False) -> None:
        """Chunk `index` of the plan `plan_epoch(seed)` would make (same members, grouped by user),
        alone; on_side: queued on the split refresh's side stream behind the sort in flight."""
        if not on_side:
            self._sync_stream()
        native.check(self._lib.bpr_plan_chunk(self._ctx, users.data_ptr(), pos.data_ptr(), users.numel(),
                                              chunk, seed, index, out[0].data_ptr(), out[1].data_ptr(),
                                              int(on_side)))

    def flush_lazy(self) -> None:
        self._sync_stream()
        native.check(self._lib.bpr_flush_lazy(self._ctx))

    def flush_items(self) -> None:
        """flush_lazy for the item table (+ bias) only (before an item reconciliation)."""
        self._sync_stream()
        native.check(self._lib.bpr_flush_items(self._ctx))

    @property
    def step_count(self) -> int:
        v = ctypes.c_int64()
        native.check(self._lib.bpr_get_step_host(self._ctx, ctypes.byref(v)))
        return v.value

    def set_step(self, step: int) -> None:
        native.check(self._lib.bpr_set_step(self._ctx, step))

    def set_sampler_iter(self, iteration: int) -> None:
        """Batch counter of the train_strict loop (AdaptiveSampler._iteration_cnt)."""
        native.check(self._lib.bpr_set_sampler_iter(self._ctx, iteration))

    # ---- measurement ------------------------------------------------------------------------
    def timing_enable(self, on=True) -> None:
        """hipEvent timing of the dominant kernel: True / 1 = every launch, N > 1 = every N-th launch
        (the event records idle the stream for a few microseconds), False / 0 = off."""
        native.check(self._lib.bpr_timing_enable(self._ctx, int(on)))

    def timing_read(self) -> tuple[float, int]:
        ms, n = ctypes.c_double(), ctypes.c_int64()
        native.check(self._lib.bpr_timing_read_host(self._ctx, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
