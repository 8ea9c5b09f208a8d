#!/usr/bin/env python
"""What does `item_filter=` cost or save in `rank_items` (`bpr_rank_rows_filtered`) and in `similar_items`
(`bpr_neighbors_rows_filtered`)?  The ML-20M shape of tools/rank_probe.py (10,000 eval users of the synthetic ML-20M
data, I = 20,109, d = 128, its seen CSR and held-out targets) and of tools/similar_probe.py (all 20,108 items as
queries, k = 100, cosine).  Filters: none, all ones, 10 % of the ids at random and a contiguous block of 5 % of the
ids (the tile-skip case).  One process, hipEvents around each call after a warm-up, median (min .. max) of REPS runs.
The all-ones line is to be read against the unfiltered line of the same run: whether its median falls inside that
line's own min .. max is written down, not asserted.  k_rank had no committed speed measurement before this file: the
unfiltered `rank_items` line is the first.
Usage: python tools/rank_filter_probe.py [--reps 5] [--out profiles/rank_filter_probe.txt]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.datasets import synthetic  # noqa: E402
from revisit_bpr.item_filter import pack_item_filter  # noqa: E402
from revisit_bpr.ranks import rank_items, slices  # noqa: E402
from revisit_bpr.similar import similar_items  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--users", type=int, default=10_000)
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "rank_filter_probe.txt"))
opt = ap.parse_args()
dev = torch.device("cuda")

data = synthetic.generate_named("ml-20m", eval_users=opt.users, seed=3)
U, I, d, k = data.num_users, data.num_items, 128, 100
g = torch.Generator().manual_seed(1)
P = ((torch.rand(U, d, generator=g) - 0.5) / d).to(dev)
Q = ((torch.rand(I, d, generator=g) - 0.5) / d).to(dev)
t = {n: torch.from_numpy(getattr(data, n)).to(dev) for n in ("eval_users", "eval_indptr", "eval_items", "indptr", "indices")}
E = t["eval_users"].numel()
ptr = (t["eval_indptr"][:E + 1] - t["eval_indptr"][0]).contiguous()
items = t["eval_items"][int(t["eval_indptr"][0]):int(t["eval_indptr"][E])].to(torch.int32).contiguous()
queries = torch.arange(1, I, dtype=torch.int32, device=dev)


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
    return s[len(s) // 2], s[0], s[-1]


gm = torch.Generator(device=dev).manual_seed(3)
draw = torch.rand(I, device=dev, generator=gm)
block = torch.zeros(I, dtype=torch.bool, device=dev)
block[8_000:8_000 + I // 20] = True
cases = [("no filter", None), ("all ones", torch.ones(I, dtype=torch.bool, device=dev)),
         ("10 % at random", draw < 0.1), ("5 % contiguous block", block)]

lines = [f"device {torch.cuda.get_device_name(0)}; I = {I}, d = {d}; ms, median (min .. max) of {opt.reps} after a "
         f"warm-up",
         f"rank_items: E = {E} users, {items.numel()} targets, item slices chosen {slices(E, I, d)}; "
         f"similar_items: n = {queries.numel()} queries, k = {k}, cosine",
         "k_rank had no committed timing before this file: the `no filter` line of rank_items is the first.",
         f"{'filter':22s} | {'eligible':>8s} | {'tiles':>9s} | {'rank_items':>30s} | {'similar_items':>30s}"]
plain = {}
for name, mask in cases:
    f = None if mask is None else pack_item_filter(I, mask=mask)
    if mask is None:
        eligible, tiles = I - 1, f"{-(-I // 128)}/{-(-I // 128)}"
    else:
        m = mask.clone()
        m[0] = False
        pad = torch.zeros(-(-I // 128) * 128, dtype=torch.bool, device=dev)
        pad[:I] = m
        eligible, tiles = int(m.sum()), f"{int(pad.view(-1, 128).any(dim=1).sum())}/{-(-I // 128)}"
    r = measure(lambda: rank_items(P, Q, None, t["eval_users"], ptr, items, t["indptr"], t["indices"], item_filter=f))
    s = measure(lambda: similar_items(Q, queries, k, "cosine", check_rows=False, item_filter=f))
    lines.append(f"{name:22s} | {eligible:8d} | {tiles:>9s} | {r[0]:8.3f} ({r[1]:8.3f} .. {r[2]:8.3f})    | "
                 f"{s[0]:8.3f} ({s[1]:8.3f} .. {s[2]:8.3f})")
    if mask is None:
        plain = {"rank_items": r, "similar_items": s}
    elif name == "all ones":
        for what, v in (("rank_items", r), ("similar_items", s)):
            lo, hi = plain[what][1], plain[what][2]
            lines.append(f"  {what}: the all-ones median {v[0]:.3f} ms is "
                         f"{'inside' if lo <= v[0] <= hi else 'OUTSIDE'} the unfiltered run's min .. max "
                         f"({lo:.3f} .. {hi:.3f})")
text = "\n".join(lines)
print(text)
Path(opt.out).write_text(text + "\n")
