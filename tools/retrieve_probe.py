#!/usr/bin/env python
"""What does a deep first stage cost through the fused kernel (`revisit_bpr.retrieve`, csrc/bpr_retrieve.hip) and
through the torch composition — P[users] @ Q.T, the seen scatter, torch.topk(k), in blocks of 4,096 users, as
`evaluation.evaluate_topk` — at the ML-20M shape (138,493 users x 20,109 items, d = 128) for k = 128, 256, 512,
1,024?  At k = 128 also against `recommend` (k_topk).  Trained-scale tables ((rand - 0.5) / d), a seen CSR of the
dataset's mean row length.  One process, the forms alternately, hipEvents around each call after a warm-up, median
and range of REPS runs.  Usage: python tools/retrieve_probe.py [--reps 5] [--n 138493,4096] [--ks 128,256,512,1024]
[--out profiles/retrieve_probe.txt]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.recommend import recommend  # noqa: E402
from revisit_bpr.retrieve import retrieve, slices, workspace_bytes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--block", type=int, default=4096)
ap.add_argument("--n", type=str, default="138493,4096", help="comma-separated user counts")
ap.add_argument("--ks", type=str, default="128,256,512,1024")
ap.add_argument("--out", type=str, default="", help="also write the table to this file")
opt = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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
    """the ranking part of evaluation.evaluate_topk"""
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
    return f"{s[len(s) // 2]:10.3f}  {s[0]:9.3f} .. {s[-1]:9.3f}", s[len(s) // 2]


U, I, d, mean_seen = 138_493, 20_109, 128, 144
say(f"device {torch.cuda.get_device_name(0)}; ML-20M shape U={U} I={I} d={d}; reps {opt.reps}; composition block "
    f"{opt.block}; times in ms: median  min .. max")
say(f"{'n':>7s} {'k':>5s} {'slices':>6s} {'ws MiB':>7s} | {'retrieve':>33s} | {'composition':>33s} | "
    f"{'comp/retr':>9s} | {'recommend (k = 128)':>33s} | same items")
P, Q, indptr, indices = tables(U, I, d, mean_seen, seed=1)
perm = torch.randperm(U, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(torch.int32)
for n in (int(x) for x in opt.n.split(",")):
    users = perm[:n].contiguous()
    for k in (int(x) for x in opt.ks.split(",")):
        forms = [lambda: retrieve(P, Q, None, users, k, indptr, indices, check_users=False)[0],
                 lambda: composition(P, Q, users, k, indptr, indices, opt.block)]
        if k <= 128:
            forms.append(lambda: recommend(P, Q, None, users, k, indptr, indices, check_users=False)[0])
        for _ in range(2):  # warm-up of every form
            outs = [f() for f in forms]
        torch.cuda.synchronize()
        same = float((outs[0].long() == outs[1]).float().mean())
        if k <= 128:
            assert torch.equal(outs[0], outs[2])
        ms = [[] for _ in forms]
        for _ in range(opt.reps):
            for j, f in enumerate(forms):
                ms[j].append(timed(f)[0])
        del outs
        (rt, rm), (ct, cm) = stats(ms[0]), stats(ms[1])
        s = slices(n, I, d, k)
        say(f"{n:7d} {k:5d} {s:6d} {workspace_bytes(n, I, d, k, s) / 2 ** 20:7.1f} | {rt} | {ct} | {cm / rm:9.2f} | "
            f"{stats(ms[2])[0] if k <= 128 else '':>33s} | {same:.4f}")
if opt.out:
    Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
    Path(opt.out).write_text("\n".join(lines) + "\n")
