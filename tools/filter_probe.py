#!/usr/bin/env python
"""What does `recommend(item_filter=...)` cost (csrc/bpr_item_filter.h, `bpr_topk_rows_filtered`) next to the two
things a caller could do without it — the unfiltered call followed by a torch post-filter (which returns FEWER than k
items; it is timed, not recommended), and `rerank` with the eligible ids as one shared candidate list?  The ML-20M
shape of tools/recommend_probe.py: I = 20,109, d = 128, k = 100, n = 10,000 users, trained-scale tables, a seen CSR of
the dataset's mean row length.  Filters: none, all ones, 50 % / 10 % / 1 % of the ids drawn at random, and a contiguous
block of 5 % of the ids (the tile-skip case).  One process, hipEvents around each call after a warm-up, median
(min .. max) of REPS runs.  Usage: python tools/filter_probe.py [--reps 5] [--out profiles/filter_probe.txt]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.item_filter import pack_item_filter, unpack_item_filter  # noqa: E402
from revisit_bpr.recommend import recommend  # noqa: E402
from revisit_bpr.rerank import rerank  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "filter_probe.txt"))
opt = ap.parse_args()
dev = torch.device("cuda")
U, I, d, k, n, mean_seen = 138_493, 20_109, 128, 100, 10_000, 144

g = torch.Generator(device=dev).manual_seed(1)
P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
cnt = torch.randint(1, 2 * mean_seen, (U,), device=dev, generator=g)
indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
stride = (I - 1) // (2 * mean_seen)  # sorted, distinct items per row (tools/recommend_probe.py)
offs = torch.arange(int(indptr[-1]), device=dev) - torch.repeat_interleave(indptr[:-1], cnt)
base = torch.repeat_interleave(torch.randint(0, stride, (U,), device=dev, generator=g), cnt)
indices = (1 + stride * offs + base).to(torch.int32)
users = torch.randperm(U, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(torch.int32)[:n]
users = users.contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(fn):
    fn()
    torch.cuda.synchronize()  # the warm-up
    s = sorted(timed(fn) for _ in range(opt.reps))
    return f"{s[len(s) // 2]:8.3f} ({s[0]:8.3f} .. {s[-1]:8.3f})"


def post_filter(mask):
    """the unfiltered call, then ineligible ids masked out and the row compacted to the front (stable sort)"""
    items, scores = recommend(P, Q, None, users, k, indptr, indices)
    keep = mask[items.long().clamp(min=0)] & (items >= 0)
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
    items = torch.where(keep, items, torch.full_like(items, -1)).gather(1, order)
    scores = torch.where(keep, scores, torch.full_like(scores, float("-inf"))).gather(1, order)
    return items, scores, keep.sum(dim=1)


gm = torch.Generator(device=dev).manual_seed(3)
draw = torch.rand(I, device=dev, generator=gm)
block = torch.zeros(I, dtype=torch.bool, device=dev)
block[8_000:8_000 + I // 20] = True
cases = [("no filter", None), ("all ones", torch.ones(I, dtype=torch.bool, device=dev)),
         ("50 % at random", draw < 0.5), ("10 % at random", draw < 0.1), ("1 % at random", draw < 0.01),
         ("5 % contiguous block", block)]

lines = [f"device {torch.cuda.get_device_name(0)}; I = {I}, d = {d}, k = {k}, n = {n}; ms, median (min .. max) of "
         f"{opt.reps} after a warm-up",
         f"{'filter':22s} | {'eligible':>8s} | {'tiles':>9s} | {'recommend(item_filter)':>30s} | "
         f"{'recommend + torch post-filter':>30s} | {'rows short of k':>15s} | {'rerank, shared list':>30s} | same"]
for name, mask in cases:
    f = None if mask is None else pack_item_filter(I, mask=mask)
    if f is not None:
        assert torch.equal(unpack_item_filter(f, I), mask)
        words = f.view(-1, 4)
        tiles = f"{int((words != 0).any(dim=1).sum())}/{words.shape[0]}"
    else:
        tiles = f"{(I + 127) // 128}/{(I + 127) // 128}"
    mask_or_all = torch.ones(I, dtype=torch.bool, device=dev) if mask is None else mask
    fused = measure(lambda: recommend(P, Q, None, users, k, indptr, indices, item_filter=f))
    post = measure(lambda: post_filter(mask_or_all))
    want = recommend(P, Q, None, users, k, indptr, indices, item_filter=f)
    pi, ps, have = post_filter(mask_or_all)
    short = int((have < torch.minimum(torch.tensor(k, device=dev), (want[0] >= 0).sum(dim=1))).sum())
    # where the post-filter has items, they are the filtered call's prefix
    cols = torch.arange(k, device=dev).unsqueeze(0) < have.unsqueeze(1)
    same = bool((torch.where(cols, pi, want[0]) == want[0]).all())
    rr = f"{'-':>30s}"
    if name in ("1 % at random", "5 % contiguous block"):
        ids = torch.nonzero(mask).reshape(-1).to(torch.int32)
        rr = measure(lambda: rerank(P, Q, None, users, ids, k, None, indptr, indices))
        ri = rerank(P, Q, None, users, ids, k, None, indptr, indices)
        same = same and bool(torch.equal(ri[0], want[0]) and torch.equal(ri[1], want[1]))
    lines.append(f"{name:22s} | {int(mask_or_all[1:].sum()):8d} | {tiles:>9s} | {fused:>30s} | {post:>30s} | "
                 f"{short:15d} | {rr:>30s} | {same}")
    print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
Path(opt.out).write_text(text)
print(text)
