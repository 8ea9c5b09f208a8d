#!/usr/bin/env python
"""What does "score these users on these candidates and keep the k best" cost through the fused kernel
(`revisit_bpr.rerank`, csrc/bpr_rerank.hip) and through the composition it replaces — Q[cand] gathered to [rows, C, d],
multiplied by P[users] and summed, + bias, id 0 and the seen items masked through a dense [U, I] seen matrix, torch.topk
— in blocks of rows whose gathered buffer stays under --block-bytes?  ML-20M shape (I = 20,109, d = 128) with
n in {1, 256, 10,000} rows x C in {100, 1,000, I - 1} candidates per row, and one MSD-shape line (I = 41,140, d = 256).
Candidates are uniform random ids (a CSR of equal rows), every user has seen ~ 144 random items, k = 10, trained-scale
tables ((rand - 0.5) / d).  The fused call is timed in the layout the plan chooses and in the other one, since the
threshold between them has not been tuned.  One process, the forms alternately, hipEvents around each call after a
warm-up, median and range of REPS runs.  GB/s is nnz * (4 d + 4) bytes over the fused median, against 8 TB/s.
Usage: python tools/rerank_probe.py [--reps 5] [--k 10] [--ns 1,256,10000] [--out profiles/rerank_probe.txt]
(profiles/rerank_probe_rows.txt: --ns 512,1024,2048,4096, the row counts between which the plan changes layout)"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr import rerank as rr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--ns", type=str, default="1,256,10000", help="row counts of the ML-20M lines")
ap.add_argument("--block-bytes", type=int, default=1 << 30)
ap.add_argument("--out", type=str, default="", help="also write the table to this file")
opt = ap.parse_args()
dev = torch.device("cuda")
PEAK = 8e12  # bytes/s of HBM
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


@torch.no_grad()
def composition(P, Q, b, users, cand, seen, k, block):
    out = []
    for lo in range(0, users.numel(), block):
        u, c = users[lo:lo + block].long(), cand[lo:lo + block].long()
        s = (Q[c] * P[u][:, None]).sum(-1) + b[c]
        s.masked_fill_(seen[u[:, None], c] | (c == 0), float("-inf"))
        top = torch.topk(s, k, dim=1)
        out.append(torch.gather(c, 1, top.indices))
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


say(f"device {torch.cuda.get_device_name(0)}; reps {opt.reps}; k {opt.k}; composition blocks of <= {opt.block_bytes} "
    f"gathered bytes; layouts: 1 = wave per row (tile 64), 2 = workgroup per row (tile 256)")
say(f"{'shape':22s} {'n':>6s} {'C':>6s} | {'layout':>6s} {'fused ms (median  min .. max)':>30s} {'GB/s':>8s} {'of 8TB/s':>8s} | "
    f"{'other layout ms (median  min .. max)':>36s} | {'composition ms (median  min .. max)':>35s} | {'comp/fused':>10s} | "
    f"{'same ids':>8s}")
SHAPES = [("ML-20M I=20109 d=128", 20_109, 128, n, C) for n in map(int, opt.ns.split(",")) for C in (100, 1_000, 20_108)]
SHAPES.append(("MSD I=41140 d=256", 41_140, 256, 10_000, 1_000))
U = 10_000
for name, I, d, n, C in SHAPES:
    g = torch.Generator(device=dev).manual_seed(1)
    P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
    Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
    b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
    seen = torch.rand(U, I, device=dev, generator=g) < 144 / I
    seen[:, 0] = False
    cnt = seen.sum(1)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
    indices = seen.nonzero()[:, 1].to(torch.int32).contiguous()  # row-major: sorted inside a row
    users = torch.randperm(U, device=dev, generator=g)[:n].to(torch.int32)
    cand = torch.randint(0, I, (n, C), device=dev, generator=g, dtype=torch.int32)
    cptr = torch.arange(n + 1, device=dev, dtype=torch.int64) * C
    flat = cand.reshape(-1)
    k = min(opt.k, C)
    auto = rr.layout_of(n, d, k, C)[0]
    other = rr.LAYOUT_WG if auto == rr.LAYOUT_WAVE else rr.LAYOUT_WAVE
    block = max(1, opt.block_bytes // (C * d * 4))

    def fused(layout):
        return rr.rerank(P, Q, b, users, flat, k, cptr, indptr, indices, layout=layout, check_users=False)[0]

    comp = lambda: composition(P, Q, b, users, cand, seen, k, block)  # noqa: E731
    for _ in range(2):  # warm-up of all three
        fi, fo, ci = fused(auto), fused(other), comp()
    torch.cuda.synchronize()
    assert torch.equal(fi, fo)
    same = float((fi.long() == ci).float().mean())  # (ties between equal scores may fall the other way)
    tf, to, tc = [], [], []
    for _ in range(opt.reps):
        tf.append(timed(lambda: fused(auto))[0])
        to.append(timed(lambda: fused(other))[0])
        tc.append(timed(comp)[0])
    rate = n * C * (4 * d + 4) / (stats(tf)[0] * 1e-3)
    say(f"{name:22s} {n:6d} {C:6d} | {auto:6d} {cell(tf)} {rate / 1e9:8.1f} {100 * rate / PEAK:7.2f}% | {cell(to):>36s} | "
        f"{cell(tc):>35s} | {stats(tc)[0] / stats(tf)[0]:10.2f} | {same:8.4f}")
    del P, Q, b, seen, cand, flat
if opt.out:
    Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
    Path(opt.out).write_text("\n".join(lines) + "\n")
