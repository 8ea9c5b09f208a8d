#!/usr/bin/env python
"""What does the draw cost on top of the sweep?  The fused sampler (`revisit_bpr.sample.sample_items`,
csrc/bpr_sample.hip) against `recommend` (csrc/bpr_topk.hip) at the same k, on the shapes of tools/recommend_probe.py:
ML-20M (I = 20,109, d = 128, k = 100; n = 1, 256, 10,000, all 138,493 users) and MSD (I = 41,140, d = 256,
n = 10,000), trained-scale tables, a seen CSR of the dataset's mean row length.  Per shape: `recommend`, the sampler,
and the sampler with keys and log_z.  One process, the three forms alternately, hipEvents around each call after a
warm-up, median and range of REPS runs.  Usage: python tools/sample_probe.py [--reps 5] [--slices 0]
[--only 10000,138493] [--out profiles/sample_probe.txt]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.recommend import recommend  # noqa: E402
from revisit_bpr.sample import sample_items  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--slices", type=int, default=0)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--only", type=str, default="", help="comma-separated n: only these rows of the ML-20M shape")
ap.add_argument("--out", type=str, default="", help="also write the table to this file")
opt = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def tables(U, I, d, mean_seen, seed):
    """tools/recommend_probe.py's tables"""
    g = torch.Generator(device=dev).manual_seed(seed)
    P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
    Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
    cnt = torch.randint(1, 2 * mean_seen, (U,), device=dev, generator=g)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
    stride = (I - 1) // (2 * mean_seen)
    offs = torch.arange(int(indptr[-1]), device=dev) - torch.repeat_interleave(indptr[:-1], cnt)
    base = torch.repeat_interleave(torch.randint(0, stride, (U,), device=dev, generator=g), cnt)
    indices = (1 + stride * offs + base).to(torch.int32)
    assert int(indices.max()) < I
    return P, Q, indptr, indices


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    s = sorted(ms)
    return s[len(s) // 2], s[0], s[-1]


say(f"device {torch.cuda.get_device_name(0)}; reps {opt.reps}; item_slices {opt.slices}; T {opt.temperature}")
say(f"{'shape':28s} {'n':>8s} | {'recommend ms (median min..max)':>34s} | {'sample ms':>30s} | {'x':>5s} | "
    f"{'sample + keys + log_z ms':>30s} | {'x':>5s}")
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
        kw = dict(item_slices=opt.slices, check_users=False)
        forms = (lambda: recommend(P, Q, None, users, k, indptr, indices, **kw),
                 lambda: sample_items(P, Q, None, users, k, indptr, indices, temperature=opt.temperature, seed=1, **kw),
                 lambda: sample_items(P, Q, None, users, k, indptr, indices, temperature=opt.temperature, seed=1,
                                      return_keys=True, return_log_z=True, **kw))
        for _ in range(2):  # warm-up of all
            for f in forms:
                f()
        torch.cuda.synchronize()
        ms = [[], [], []]
        for _ in range(opt.reps):
            for j, f in enumerate(forms):
                ms[j].append(timed(f))
        (rm, r0, r1), (sm_, s0, s1), (lm, l0, l1) = (stats(m) for m in ms)
        say(f"{name:28s} {n:8d} | {rm:12.3f} {r0:9.3f} ..{r1:9.3f} | {sm_:10.3f} {s0:8.3f} ..{s1:8.3f} | "
            f"{sm_ / rm:5.2f} | {lm:10.3f} {l0:8.3f} ..{l1:8.3f} | {lm / rm:5.2f}")
    del P, Q, indptr, indices
if opt.out:
    Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
    Path(opt.out).write_text("\n".join(lines) + "\n")
