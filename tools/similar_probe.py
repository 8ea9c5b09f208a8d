#!/usr/bin/env python
"""What does "the k most similar items" cost through the fused kernel (`revisit_bpr.similar`, csrc/bpr_neighbors.hip)
and through the composition it replaces — F.normalize (cosine only), Qn[rows] @ Qn.T in blocks of 4,096 queries, the
query itself and id 0 masked, torch.topk(k) — at the ML-20M shape (I = 20,109, d = 128; n = 1, 256 and all 20,108
items) and at the MSD shape (I = 41,140, d = 256; n = 10,000), k = 100, both metrics?  A third column runs `k_topk`
(revisit_bpr.recommend) on the same table and queries with no seen CSR: the same tiling and selection whose step (C)
then searches empty rows, to set beside DESIGN 4.6's figures with a CSR.  Trained-scale tables ((rand - 0.5) / d).
One process, the forms alternately, hipEvents around each call after a warm-up, median and range of REPS runs.
Usage: python tools/similar_probe.py [--reps 5] [--slices 0] [--out profiles/similar_probe.txt]"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.recommend import recommend  # noqa: E402
from revisit_bpr.similar import similar_items  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--slices", type=int, default=0)
ap.add_argument("--block", type=int, default=4096)
ap.add_argument("--out", type=str, default="", help="also write the table to this file")
opt = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


@torch.no_grad()
def composition(Q, rows_all, k, metric, block):
    Qn = F.normalize(Q, dim=1) if metric == "cosine" else Q
    out = []
    for lo in range(0, rows_all.numel(), block):
        rows = rows_all[lo:lo + block].long()
        S = Qn[rows] @ Qn.T
        S[torch.arange(rows.numel(), device=dev), rows] = -1e13
        S[:, 0] = -1e13
        out.append(torch.topk(S, k, dim=1).indices)
    return torch.cat(out)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


def cell(ms):
    m, lo, hi = stats(ms)
    return f"{m:9.3f} {lo:9.3f} ..{hi:9.3f}"


say(f"device {torch.cuda.get_device_name(0)}; reps {opt.reps}; composition block {opt.block}; item_slices {opt.slices}")
say(f"{'shape':28s} {'metric':>6s} {'n':>6s} | {'fused ms (median  min .. max)':>30s} | "
    f"{'composition ms (median  min .. max)':>35s} | {'comp/fused':>10s} | {'same ids':>8s} | "
    f"{'k_topk, no CSR, ms (median  min .. max)':>39s}")
for name, I, d, k, ns in (("ML-20M I=20109 d=128 k=100", 20_109, 128, 100, (1, 256, 20_108)),
                          ("MSD I=41140 d=256 k=100", 41_140, 256, 100, (10_000,))):
    g = torch.Generator(device=dev).manual_seed(1)
    Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
    perm = (1 + torch.randperm(I - 1, device=dev, generator=torch.Generator(device=dev).manual_seed(2))).to(torch.int32)
    for metric in ("cosine", "dot"):
        for n in ns:
            rows = perm[:n].contiguous()
            fused = lambda: similar_items(Q, rows, k, metric, item_slices=opt.slices, check_rows=False)[0]  # noqa: E731
            comp = lambda: composition(Q, rows, k, metric, opt.block)  # noqa: E731
            topk = lambda: recommend(Q, Q, None, rows, k, item_slices=opt.slices, check_users=False)[0]  # noqa: E731
            for _ in range(2):  # warm-up of all three
                fi, ci, _ = fused(), comp(), topk()
            torch.cuda.synchronize()
            same = float((fi.long() == ci).float().mean())
            tf, tc, tt = [], [], []
            for _ in range(opt.reps):
                tf.append(timed(fused)[0])
                tc.append(timed(comp)[0])
                tt.append(timed(topk)[0])
            say(f"{name:28s} {metric:>6s} {n:6d} | {cell(tf)} | {cell(tc):>35s} | {stats(tc)[0] / stats(tf)[0]:10.2f} | "
                f"{same:8.4f} | {cell(tt):>39s}")
    del Q
if opt.out:
    Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
    Path(opt.out).write_text("\n".join(lines) + "\n")
