#!/usr/bin/env python
"""What does one evaluation of the reference's ML-20M protocol (10,000 held-out users x 20,108 items; the data of
tools/eval_probe.py) cost through `evaluate_ranked(auc=True)` — one fused ranking pass, csrc/bpr_rank.hip — against
the dense path `evaluate_topk(auc=True)` and against `evaluate_fused` (top-K kernel: no AUC, k <= 128), and where
does the time of the ranked form go (`rank_items` alone, the kernels of `bpr_rank_rows` alone for 1 and the
library's choice of item slices)?  One process, the forms alternately, hipEvents around each call after a warm-up,
median and range of REPS runs.  Usage: python tools/rank_probe.py [--reps 7] [--users 10000]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.datasets import synthetic  # noqa: E402
from revisit_bpr.evaluation import evaluate_fused, evaluate_ranked, evaluate_topk  # noqa: E402
from revisit_bpr.ranks import rank_items, slices  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--users", type=int, default=10_000)
ap.add_argument("--block", type=int, default=4096)
opt = ap.parse_args()
dev = torch.device("cuda")

data = synthetic.generate_named("ml-20m", eval_users=opt.users, seed=3)
U, I, d = data.num_users, data.num_items, 128
g = torch.Generator().manual_seed(1)
P = ((torch.rand(U, d, generator=g) - 0.5) / d).to(dev)
Q = ((torch.rand(I, d, generator=g) - 0.5) / d).to(dev)
t = {k: torch.from_numpy(getattr(data, k)).to(dev) for k in ("eval_users", "eval_indptr", "eval_items", "indptr", "indices")}
args = (P, Q, None, t["eval_users"], t["eval_indptr"], t["eval_items"], t["indptr"], t["indices"])
ks = (5, 10, 20, 50, 100)
E = t["eval_users"].numel()
ptr = (t["eval_indptr"][:E + 1] - t["eval_indptr"][0]).contiguous()
items = t["eval_items"][int(t["eval_indptr"][0]):int(t["eval_indptr"][E])].to(torch.int32).contiguous()
cnt = ptr[1:] - ptr[:-1]
print(f"device {torch.cuda.get_device_name(0)}; reps {opt.reps}; E {E} users, I {I}, d {d}; targets {items.numel()} "
      f"(per user: mean {float(cnt.float().mean()):.1f}, max {int(cnt.max())}); dense block {opt.block}; "
      f"item slices chosen {slices(E, I, d)}")

forms = {
    "evaluate_ranked(auc=True)": lambda: evaluate_ranked(*args, ks=ks, auc=True),
    "evaluate_ranked(auc, extra, ks to 1000)": lambda: evaluate_ranked(*args, ks=ks + (200, 1000), auc=True, extra=True),
    "evaluate_topk(auc=True)": lambda: evaluate_topk(*args, ks=ks, block=opt.block, auc=True),
    "evaluate_topk (no auc)": lambda: evaluate_topk(*args, ks=ks, block=opt.block),
    "evaluate_fused (no auc)": lambda: evaluate_fused(*args, ks=ks),
    "  rank_items alone": lambda: rank_items(P, Q, None, t["eval_users"], ptr, items, t["indptr"], t["indices"]),
    "  rank_items, no user check, 1 slice": lambda: rank_items(P, Q, None, t["eval_users"], ptr, items, t["indptr"],
                                                             t["indices"], item_slices=1, check_users=False),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


last = {}
for _ in range(2):  # warm-up of every form
    for name, fn in forms.items():
        last[name] = fn()
torch.cuda.synchronize()
ms = {name: [] for name in forms}
for _ in range(opt.reps):
    for name, fn in forms.items():
        ms[name].append(timed(fn)[0])
print(f"{'form':44s} | {'ms (median  min .. max)':>32s}")
for name, v in ms.items():
    s = sorted(v)
    print(f"{name:44s} | {s[len(s) // 2]:12.3f}  {s[0]:8.3f} .. {s[-1]:8.3f}")
r, k = last["evaluate_ranked(auc=True)"], last["evaluate_topk(auc=True)"]
print("largest difference of a shared key, ranked - dense:", max(abs(r[n] - k[n]) for n in k),
      "| auc", r["auc"], k["auc"], "| ndcg@100", r["ndcg@100"], k["ndcg@100"])
