"""Eval path (PyTorch-ROCm): score every item for a block of users, mask what the user has seen,
feed the streaming metrics.  Value-identical to the reference's eval loop (example.py:195-230;
experiments/bpr/exp.py:369-374): logits = P[users] Qᵀ (+ item bias), seen items and item 0 set to
−1e13, every metric consumes (logits, target).  One dense GEMM per block (rocBLAS/hipBLASLt via
torch — the only MFMA-shaped work in the whole path) instead of a [B, I, d] gather + einsum.
"""
from __future__ import annotations

from typing import Mapping

import torch

from revisit_bpr.metrics import Metric


@torch.no_grad()
def evaluate(P: torch.Tensor, Q: torch.Tensor, item_bias, eval_users: torch.Tensor,
             eval_indptr: torch.Tensor, eval_items: torch.Tensor, seen_indptr: torch.Tensor,
             seen_indices: torch.Tensor, metrics: Mapping[str, Metric], block: int = 2048) -> dict:
    """eval_users [E]; eval_indptr [E+1] / eval_items: held-out targets per eval user (CSR);
    seen_indptr [U+1] / seen_indices: items to mask per user (CSR).  Returns {name: float}."""
    dev = P.device
    I = Q.shape[0]
    for m in metrics.values():
        m.reset()
    E = eval_users.numel()
    for lo in range(0, E, block):
        hi = min(lo + block, E)
        users = eval_users[lo:hi].long()
        logits = P[users] @ Q.T
        if item_bias is not None:
            logits += item_bias
        n = hi - lo
        rows = torch.arange(n, device=dev)
        # targets
        t_lo, t_hi = eval_indptr[lo:hi], eval_indptr[lo + 1:hi + 1]
        t_cnt = (t_hi - t_lo)
        target = torch.zeros(n, I, device=dev)
        if int(t_cnt.sum()) > 0:
            r = torch.repeat_interleave(rows, t_cnt)
            target[r, eval_items[int(t_lo[0]):int(t_hi[-1])].long()] = 1.0
        # seen mask
        s_lo, s_hi = seen_indptr[users], seen_indptr[users + 1]
        s_cnt = s_hi - s_lo
        if int(s_cnt.sum()) > 0:
            r = torch.repeat_interleave(rows, s_cnt)
            offs = torch.arange(int(s_cnt.sum()), device=dev) - torch.repeat_interleave(
                torch.cumsum(s_cnt, 0) - s_cnt, s_cnt)
            cols = seen_indices[(torch.repeat_interleave(s_lo, s_cnt) + offs)].long()
            logits[r, cols] = -1e13
        logits[:, 0] = -1e13
        for m in metrics.values():
            m(logits, target)
    return {k: float(m.get_metric()) for k, m in metrics.items()}


@torch.no_grad()
def evaluate_topk(P: torch.Tensor, Q: torch.Tensor, item_bias, eval_users: torch.Tensor,
                  eval_indptr: torch.Tensor, eval_items: torch.Tensor, seen_indptr: torch.Tensor,
                  seen_indices: torch.Tensor, ks=(5, 10, 20, 50, 100), block: int = 8192,
                  auc: bool = False) -> dict:
    """NDCG / Recall / Precision at every k in `ks` from ONE top-max(ks) per block of users (the
    reference runs a full argsort of I scores per metric object: 14 sorts per batch,
    experiments/bpr/exp.py:369-374 + metrics/metric.py:110-113).  Same values as the metric classes
    (tests/test_gpu_api.py::test_evaluate_topk_equals_metric_classes).  `auc=True` adds the
    ROC-AUC of the reference's RocAucMany (metrics/auc.py:70-130: all positive / negative pairs of a
    row) from the same block of scores: on a ROCm device `bpr_auc_rows` (csrc/bpr_eval.hip, r6: one pass over the
    scores, the positives ranked in LDS), else by rank sums after one sort per block — instead of the [B, I, I]
    comparison.  For `auc` a user's targets are a SET: a target counts once however often the eval CSR lists it, on
    either device (the kernel wants unique ids: the repeats are dropped from a sorted key list before the block loop,
    one pass over the targets, not over the scores); a pair with a NaN score on either side is not a win.  `n_pos` of
    recall and ndcg stays the listed count (tests/rank_model.py)."""
    from revisit_bpr.metrics.auc import RocAucManySlow

    auc_metric = RocAucManySlow() if auc else None
    auc_sum = torch.zeros((), device=P.device, dtype=torch.float32)
    lib = None
    dev = P.device
    I = Q.shape[0]
    E = eval_users.numel()
    if auc and P.is_cuda:  # r6: bpr_auc_rows — one pass over the scores instead of a sort per row
        from revisit_bpr import native

        lib = native.load()
        # the targets of the whole call as sorted keys (row * I + item), as evaluate_fused builds them, the first of
        # every run of equal keys kept: the CSR the kernel reads (u_ptr [E + 1] from 0, u_items), every id once per
        # row.  No device-to-host copy but the first one: the kept keys are scattered to their places, the repeats
        # to a spare slot behind them
        first, last = (int(v) for v in eval_indptr[[0, E]].tolist())
        total = last - first
        ptr0 = (eval_indptr[:E + 1] - first).long()
        keys = torch.repeat_interleave(torch.arange(E, device=dev), ptr0[1:] - ptr0[:-1], output_size=total) * I
        keys = torch.sort(keys + eval_items[first:last].long()).values
        keep = torch.ones(total, device=dev, dtype=torch.bool)
        keep[1:] = keys[1:] != keys[:-1]
        kept_before = torch.zeros(total + 1, device=dev, dtype=torch.int64)
        kept_before[1:] = torch.cumsum(keep, 0)
        u_ptr = kept_before[ptr0]
        u_cnt = u_ptr[1:] - u_ptr[:-1]
        u_items = torch.empty(total + 1, device=dev, dtype=torch.int32)
        u_items.scatter_(0, torch.where(keep, kept_before[:-1], total), (keys % I).to(torch.int32))
    kmax = min(max(ks), I)
    disc = 1.0 / torch.log2(torch.arange(kmax, dtype=torch.float, device=dev) + 2.0)
    sums = {f"{m}@{k}": torch.zeros((), device=dev, dtype=torch.float64)
            for k in ks for m in ("ndcg", "recall", "precision")}
    for lo in range(0, E, block):
        hi = min(lo + block, E)
        users = eval_users[lo:hi].long()
        n = hi - lo
        rows = torch.arange(n, device=dev)
        logits = P[users] @ Q.T
        if item_bias is not None:
            logits += item_bias
        s_lo, s_hi = seen_indptr[users], seen_indptr[users + 1]
        s_cnt = s_hi - s_lo
        tot = int(s_cnt.sum())
        if tot > 0:
            r = torch.repeat_interleave(rows, s_cnt)
            offs = torch.arange(tot, device=dev) - torch.repeat_interleave(
                torch.cumsum(s_cnt, 0) - s_cnt, s_cnt)
            logits[r, seen_indices[torch.repeat_interleave(s_lo, s_cnt) + offs].long()] = -1e13
        logits[:, 0] = -1e13
        t_lo, t_hi = eval_indptr[lo:hi], eval_indptr[lo + 1:hi + 1]
        t_cnt = t_hi - t_lo
        target = torch.zeros(n, I, device=dev, dtype=torch.bool)  # (1 byte per score; only the top-k look-up reads it)
        if int(t_cnt.sum()) > 0:
            target[torch.repeat_interleave(rows, t_cnt),
                   eval_items[int(t_lo[0]):int(t_hi[-1])].long()] = True
        if auc_metric is not None and lib is None:
            auc_metric(logits, target.float())
        elif auc_metric is not None:
            rows_auc = torch.full((n,), float("nan"), device=dev, dtype=torch.float32)
            if total > 0:  # (the block's rows of the unique CSR: offsets into all of u_items)
                native.check(lib.bpr_auc_rows(logits.data_ptr(), n, I, u_ptr[lo:hi + 1].data_ptr(), u_items.data_ptr(),
                                              rows_auc.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            many = u_cnt[lo:hi] > 4096  # (rows the kernel leaves to the sort-based form)
            if bool(many.any()):
                rows_auc[many] = auc_metric.compute(logits[many], target[many].float())
            auc_sum += rows_auc.sum()
        rel = torch.gather(target, 1, torch.topk(logits, kmax, dim=1).indices).float()  # [n, kmax]
        n_pos = t_cnt.float()
        gains = rel * disc
        for k in ks:
            kk = min(k, I)
            hits = rel[:, :kk].sum(1)
            ideal = torch.cumsum(disc, 0)[(n_pos.clamp(max=kk).long() - 1).clamp(min=0)]
            ideal = torch.where(n_pos > 0, ideal, torch.zeros_like(ideal))
            sums[f"ndcg@{k}"] += torch.nan_to_num(gains[:, :kk].sum(1) / ideal).double().sum()
            sums[f"recall@{k}"] += torch.nan_to_num(hits / n_pos).double().sum()
            sums[f"precision@{k}"] += (hits / kk).double().sum()
    out = {k: float(v / max(E, 1)) for k, v in sums.items()}
    if auc_metric is not None:
        out["auc"] = float(auc_metric.get_metric()) if lib is None else float(auc_sum / max(E, 1))
    return out


@torch.no_grad()
def evaluate_fused(P: torch.Tensor, Q: torch.Tensor, item_bias, eval_users: torch.Tensor,
                   eval_indptr: torch.Tensor, eval_items: torch.Tensor, seen_indptr: torch.Tensor,
                   seen_indices: torch.Tensor, ks=(5, 10, 20, 50, 100)) -> dict:
    """The NDCG / Recall / Precision keys of `evaluate_topk` from ONE `recommend` call with k = max(ks)
    (revisit_bpr/recommend.py: scores, seen mask and selection in one kernel, no [n, I] logits and no [n, I]
    target matrix).  Relevance of a returned item = membership in the user's row of the eval CSR, looked up
    through a sorted key list (row * I + item).  No AUC: that needs every score (`evaluate_topk(auc=True)`).
    max(ks) is at most 128, the kernel's largest k (larger cutoffs: `evaluate_topk`).
    k-th best ties are broken by ascending item id here and by torch.topk's choice there."""
    from revisit_bpr.recommend import recommend

    dev = P.device
    I = Q.shape[0]
    E = eval_users.numel()
    kmax = min(max(ks), I)
    if kmax > 128:
        raise ValueError(f"evaluate_fused ranks at most 128 items per user (max(ks) = {max(ks)}); "
                         "evaluate_topk has no such limit")
    items, _ = recommend(P, Q, item_bias, eval_users, kmax, seen_indptr, seen_indices)  # [E, kmax]
    t_cnt = (eval_indptr[1:E + 1] - eval_indptr[:E])
    rows = torch.arange(E, device=dev)
    keys = torch.repeat_interleave(rows, t_cnt) * I + eval_items[int(eval_indptr[0]):int(eval_indptr[E])].long()
    keys = torch.sort(keys).values
    probe = rows.unsqueeze(1) * I + items.long()  # (padding, item -1: the key of item I - 1 of the row before, or -1)
    if keys.numel() > 0:
        at = torch.searchsorted(keys, probe).clamp(max=keys.numel() - 1)
        rel = ((keys[at] == probe) & (items >= 0)).float()
    else:
        rel = torch.zeros_like(probe, dtype=torch.float)
    disc = 1.0 / torch.log2(torch.arange(kmax, dtype=torch.float, device=dev) + 2.0)
    n_pos = t_cnt.float()
    gains = rel * disc
    out = {}
    for k in ks:
        kk = min(k, I)
        hits = rel[:, :kk].sum(1)
        ideal = torch.cumsum(disc, 0)[(n_pos.clamp(max=kk).long() - 1).clamp(min=0)]
        ideal = torch.where(n_pos > 0, ideal, torch.zeros_like(ideal))
        out[f"ndcg@{k}"] = float(torch.nan_to_num(gains[:, :kk].sum(1) / ideal).double().sum() / max(E, 1))
        out[f"recall@{k}"] = float(torch.nan_to_num(hits / n_pos).double().sum() / max(E, 1))
        out[f"precision@{k}"] = float((hits / kk).double().sum() / max(E, 1))
    return out


@torch.no_grad()
def evaluate_ranked(P: torch.Tensor, Q: torch.Tensor, item_bias, eval_users: torch.Tensor,
                    eval_indptr: torch.Tensor, eval_items: torch.Tensor, seen_indptr, seen_indices,
                    ks=(5, 10, 20, 50, 100), auc: bool = False, extra: bool = False, per_user: bool = False,
                    masked_negatives: bool = True, item_filter=None):
    """The keys of `evaluate_topk` from ONE `rank_items` call (revisit_bpr/ranks.py: the exact position of every
    held-out item among its user's unseen items, no [n, I] logits, no target matrix) and segment arithmetic on
    the few numbers per target it returns.  No cutoff limit: any k in `ks` (k > I behaves as k = I, as in
    `evaluate_topk`).  A target counts once per user however often the eval CSR lists it, and a target that is
    itself not eligible (id 0, or seen by the user) counts as never retrieved.  Ties are broken by ascending item
    id, as in `evaluate_fused`.

    auc=True adds `auc`, the quantity of RocAucMany / RocAucManySlow (pairs with the positive STRICTLY above the
    negative, over positives x negatives; a user without positives gives 0 / 0 = NaN, as the metric classes).
    masked_negatives=True counts it as the reference's eval loop and `evaluate_topk(auc=True)` do: item 0 and the
    seen items carry -1e13 and are negatives below every positive (n_neg = I - T).  False: over the eligible
    items only (n_neg = I - 1 - |seen_u| - T_u; the metric classes with their `mask` argument).
    extra=True adds `mrr` (1 / (1 + best rank of a target), 0 without one) and `map@k` for every k, the
    reference's metrics/map.py with its default normalisation: sum over the targets retrieved in the top k of
    (targets retrieved up to it) / (its position), over min(n_pos, k).
    per_user=True returns (means, per-user tensors [E] by the same keys), the role of the reference's
    save_user_metrics.

    `item_filter` (None: the whole catalogue): a packed filter (revisit_bpr/item_filter.py) — quality on a segment:
    the long tail, one category, the new items.  The call then equals this function on the catalogue compacted to
    item 0 and the filter's items: a target in 1 .. I-1 whose bit is clear is dropped from its row before n_pos is
    counted (item 0 and ids out of range stay what they are without a filter: listed, never retrieved), ranks are
    among the filter's unseen items (`rank_items(item_filter=)`), and the AUC's eligible items of a user are the
    filter's items the user has not seen.  With masked_negatives=True the filtered-out items are negatives below
    every positive, exactly like item 0 and the seen ones: n_neg = I - T, as without a filter."""
    from revisit_bpr.item_filter import check_item_filter
    from revisit_bpr.ranks import rank_items

    I = Q.shape[0]
    E = eval_users.numel()
    item_filter = check_item_filter(item_filter, I)
    first, last = (int(v) for v in eval_indptr[[0, E]].tolist())
    ptr = (eval_indptr[:E + 1] - first).to(torch.int64)
    items = eval_items[first:last].to(torch.int32)
    if item_filter is not None:
        ptr, items = drop_filtered_targets(ptr, items, I, item_filter)
    rank, not_below, score = rank_items(P, Q, item_bias, eval_users, ptr, items, seen_indptr, seen_indices,
                                        item_filter=item_filter)
    n_elig = eligible_counts(I, eval_users, seen_indptr, seen_indices, item_filter)
    return ranked_metrics(rank, not_below, score, ptr, items, I, n_elig, ks=ks, auc=auc, extra=extra,
                          per_user=per_user, masked_negatives=masked_negatives)


def drop_filtered_targets(ptr: torch.Tensor, items: torch.Tensor, I: int, item_filter: torch.Tensor):
    """The target CSR (ptr int64 [E+1] from 0, items int32) without the targets in 1 .. I-1 whose bit of the packed
    `item_filter` is clear; item 0 and ids out of range stay.  Returns (ptr, items)."""
    from revisit_bpr.item_filter import unpack_item_filter

    E = ptr.numel() - 1
    elig = unpack_item_filter(item_filter, I)
    judged = (items >= 1) & (items < I)
    keep = ~judged | elig[items.long().clamp(0, I - 1)]
    rows = torch.repeat_interleave(torch.arange(E, device=ptr.device), ptr[1:] - ptr[:-1])
    cnt = torch.zeros(E, dtype=torch.int64, device=ptr.device).index_add_(0, rows, keep.to(torch.int64))
    new_ptr = torch.zeros(E + 1, dtype=torch.int64, device=ptr.device)
    new_ptr[1:] = torch.cumsum(cnt, 0)
    return new_ptr, items[keep].contiguous()


def eligible_counts(I: int, eval_users: torch.Tensor, seen_indptr, seen_indices, item_filter=None) -> torch.Tensor:
    """int64 [E]: how many items are eligible for each eval user — 1 .. I-1 without the user's seen row, and with a
    packed `item_filter` the filter's items among them, |F minus seen_u| (the filter's bits gathered at the seen
    indices and summed per row: no kernel output is needed)."""
    from revisit_bpr.item_filter import unpack_item_filter

    users = eval_users.long()
    if item_filter is None:
        n_seen = (seen_indptr[users + 1] - seen_indptr[users]) if seen_indptr is not None else torch.zeros_like(users)
        return I - 1 - n_seen
    elig = unpack_item_filter(item_filter, I).clone()
    elig[0] = False
    total = elig.sum().to(torch.int64)
    if seen_indptr is None:
        return total.expand(users.numel()).clone()
    run = torch.zeros(seen_indices.numel() + 1, dtype=torch.int64, device=elig.device)
    run[1:] = torch.cumsum(elig[seen_indices.long()].to(torch.int64), 0)
    return total - (run[seen_indptr[users + 1]] - run[seen_indptr[users]])


def ranked_metrics(rank: torch.Tensor, not_below: torch.Tensor, score: torch.Tensor, ptr: torch.Tensor,
                   items: torch.Tensor, I: int, n_elig: torch.Tensor, ks=(5, 10, 20, 50, 100), auc: bool = False,
                   extra: bool = False, per_user: bool = False, masked_negatives: bool = True):
    """`evaluate_ranked`'s arithmetic behind its `rank_items` call, on any device: (rank, not_below, score) aligned
    with the targets `items` of the rows `ptr` (int64 [E+1] from 0), the catalogue size I and `n_elig` (int64 [E],
    `eligible_counts`) -> the means, or (means, per-user tensors)."""
    dev = rank.device
    E = ptr.numel() - 1
    t_cnt = ptr[1:] - ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(E, device=dev), t_cnt)
    total = rows.numel()
    # the first listing of an id in its row
    in_range = (items >= 0) & (items < I)
    key = rows * I + items.long().clamp(0, I - 1)
    order = torch.argsort(key, stable=True)
    sk = key[order]
    lead = torch.ones(total, dtype=torch.bool, device=dev)
    lead[1:] = sk[1:] != sk[:-1]
    uniq = torch.empty_like(lead)
    uniq[order] = lead
    hit = uniq & (rank >= 0)  # targets that can be retrieved at all
    r = rank.long()

    def per_row(values):
        return torch.zeros(E, device=dev, dtype=torch.float64).index_add_(0, rows, values.double())

    n_pos = t_cnt.double()
    kmax = max(min(max(ks), I), 1)
    disc = 1.0 / torch.log2(torch.arange(kmax, dtype=torch.float, device=dev) + 2.0)
    ideal_at = torch.cumsum(disc, 0).double()
    gain = torch.where(hit, 1.0 / torch.log2(r.clamp(min=0).float() + 2.0), torch.zeros((), device=dev)).double()
    per = {}
    if extra:  # place of a retrievable target among its row's, by rank: 1 + retrievable targets in front of it
        hi_idx = torch.nonzero(hit).reshape(-1)
        o2 = hi_idx[torch.argsort(rows[hi_idx] * I + r[hi_idx])]
        m_row = per_row(hit).long()
        starts = torch.cumsum(m_row, 0) - m_row
        place = torch.zeros(total, dtype=torch.float64, device=dev)
        place[o2] = (torch.arange(o2.numel(), device=dev) - starts[rows[o2]] + 1).double()
        prec_at = place / (r.clamp(min=0) + 1).double()
        best = torch.full((E,), I, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, rows[hi_idx], r[hi_idx], reduce="amin")
        per["mrr"] = torch.where(best < I, 1.0 / (best + 1).double(), torch.zeros((), device=dev, dtype=torch.float64))
    for k in ks:
        kk = min(k, I)
        in_k = hit & (r < kk)
        hits = per_row(in_k)
        ideal = ideal_at[(n_pos.clamp(max=kk).long() - 1).clamp(min=0)]
        ideal = torch.where(n_pos > 0, ideal, torch.zeros_like(ideal))
        per[f"ndcg@{k}"] = torch.nan_to_num(per_row(torch.where(in_k, gain, torch.zeros_like(gain))) / ideal)
        per[f"recall@{k}"] = torch.nan_to_num(hits / n_pos)
        per[f"precision@{k}"] = hits / kk
        if extra:
            ap = per_row(torch.where(in_k, prec_at, torch.zeros_like(prec_at)))
            per[f"map@{k}"] = torch.nan_to_num(ap / n_pos.clamp(max=kk))
    if auc:
        n_masked = I - n_elig  # item 0, the seen items and (with a filter) the filtered-out ones
        # a retrievable target's other retrievable targets that score strictly below it: order the row's by
        # (rank), i.e. score descending; those after the last one of its score
        hi_idx = torch.nonzero(hit).reshape(-1)
        o2 = hi_idx[torch.argsort(rows[hi_idx] * I + r[hi_idx])]
        m = o2.numel()
        m_row = per_row(hit).long()
        ends = torch.cumsum(m_row, 0)  # one past the row's last place in o2
        at = torch.arange(m, device=dev)
        last_of_run = torch.ones(m, dtype=torch.bool, device=dev)
        if m > 1:
            last_of_run[:-1] = (rows[o2][1:] != rows[o2][:-1]) | (score[o2][1:] != score[o2][:-1])
        run_end = torch.where(last_of_run, at, torch.full_like(at, m))
        run_end = torch.flip(torch.cummin(torch.flip(run_end, [0]), 0).values, [0])
        tgt_below = torch.zeros(total, dtype=torch.int64, device=dev)
        tgt_below[o2] = ends[rows[o2]] - 1 - run_end
        below = n_elig[rows] - 1 - not_below.long() - tgt_below  # eligible non-targets strictly below the target
        if masked_negatives:
            out_of_play = per_row(uniq & in_range & (rank < 0)).long()  # positives among the masked entries
            below = below + torch.where(score > -1e13, (n_masked - out_of_play)[rows], torch.zeros_like(below))
            T = per_row(uniq & in_range)
            n_neg = I - T
        else:
            T = m_row.double()
            n_neg = n_elig.double() - T
        per["auc"] = per_row(torch.where(hit, below, torch.zeros_like(below))) / (T * n_neg)
    out = {k: float(v.sum() / max(E, 1)) for k, v in per.items()}
    return (out, per) if per_user else out
