#!/usr/bin/env python
"""What does a top-K recommendation cost through the fused kernel (`revisit_bpr.recommend`, csrc/bpr_topk.hip) and
through the composition `evaluate_topk` runs today — P[users] @ Q.T, the seen scatter, torch.topk(k), in blocks of
4,096 users — at the ML-20M shape (I = 20,109, d = 128, k = 100; n = 1, 256, 10,000, all 138,493 users) and at the MSD
shape (I = 41,140, d = 256, n = 10,000)?  Trained-scale tables ((rand - 0.5) / d), a seen CSR of the dataset's mean row
length.  One process, the two forms alternately, hipEvents around each call after a warm-up, median and range of
REPS runs.  Usage: python tools/recommend_probe.py [--reps 7] [--slices 0] [--only 10000,138493]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.recommend import recommend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--slices", type=int, default=0)
ap.add_argument("--block", type=int, default=4096)
ap.add_argument("--only", type=str, default="", help="comma-separated n: only these rows of the ML-20M shape")
opt = ap.parse_args()
dev = torch.device("cuda")


def tables(U, I, d, mean_seen, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
    Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
    cnt = torch.randint(1, 2 * mean_seen, (U,), device=dev, generator=g)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
    # sorted, distinct items per row: the r-th item of a row is 1 + stride r + (a per-row offset below stride)
    stride = (I - 1) // (2 * mean_seen)
    offs = torch.arange(int(indptr[-1]), device=dev) - torch.repeat_interleave(indptr[:-1], cnt)
    base = torch.repeat_interleave(torch.randint(0, stride, (U,), device=dev, generator=g), cnt)
    indices = (1 + stride * offs + base).to(torch.int32)
    assert int(indices.max()) < I
    return P, Q, indptr, indices


@torch.no_grad()
def composition(P, Q, users_all, k, indptr, indices, block):
    """the ranking part of evaluation.evaluate_topk, verbatim"""
    out = []
    for lo in range(0, users_all.numel(), block):
        users = users_all[lo:lo + block].long()
        n = users.numel()
        rows = torch.arange(n, device=dev)
        logits = P[users] @ Q.T
        s_lo, s_hi = indptr[users], indptr[users + 1]
        s_cnt = s_hi - s_lo
        tot = int(s_cnt.sum())
        if tot > 0:
            r = torch.repeat_interleave(rows, s_cnt)
            offs = torch.arange(tot, device=dev) - torch.repeat_interleave(torch.cumsum(s_cnt, 0) - s_cnt, s_cnt)
            logits[r, indices[torch.repeat_interleave(s_lo, s_cnt) + offs].long()] = -1e13
        logits[:, 0] = -1e13
        out.append(torch.topk(logits, k, dim=1).indices)
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


print(f"device {torch.cuda.get_device_name(0)}; reps {opt.reps}; composition block {opt.block}; item_slices {opt.slices}")
print(f"{'shape':34s} {'n':>8s} | {'fused ms (median  min .. max)':>32s} | {'composition ms (median  min .. max)':>36s} | "
      f"{'ratio':>6s} | same items")
for name, U, I, d, k, mean_seen, ns in (("ML-20M I=20109 d=128 k=100", 138_493, 20_109, 128, 100, 144,
                                         (1, 256, 10_000, 138_493)),
                                        ("MSD I=41140 d=256 k=100", 571_355, 41_140, 256, 100, 59, (10_000,))):
    if opt.only:
        ns = tuple(n for n in ns if str(n) in opt.only.split(",")) if U == 138_493 else ()
    if not ns:
        continue
    P, Q, indptr, indices = tables(U, I, d, mean_seen, seed=1)
    perm = torch.randperm(U, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(torch.int32)
    for n in ns:
        users = perm[:n].contiguous()
        fused = lambda: recommend(P, Q, None, users, k, indptr, indices, item_slices=opt.slices)[0]  # noqa: E731
        comp = lambda: composition(P, Q, users, k, indptr, indices, opt.block)  # noqa: E731
        for _ in range(2):  # warm-up of both
            fi, ci = fused(), comp()
        torch.cuda.synchronize()
        same = float((fi.long() == ci).float().mean())
        tf, tc = [], []
        for _ in range(opt.reps):
            tf.append(timed(fused)[0])
            tc.append(timed(comp)[0])
        (fm, f0, f1), (cm, c0, c1) = stats(tf), stats(tc)
        print(f"{name:34s} {n:8d} | {fm:12.3f}  {f0:8.3f} .. {f1:8.3f} | {cm:14.3f}  {c0:8.3f} .. {c1:8.3f} | "
              f"{cm / fm:6.2f} | {same:.4f}", flush=True)
    del P, Q, indptr, indices
