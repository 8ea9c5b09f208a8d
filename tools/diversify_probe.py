"""What the fused MMR kernel (`revisit_bpr.diversify.diversify`, csrc/bpr_diversify.hip) costs, and what it buys.

(i) Timing.  One process; per shape the fused call and the torch composition on the same inputs run alternately.  The
composition is the obvious one: gather Q[cand] into [n, C, d], normalize (cosine), `bmm` into [n, C, C], then k
rounds of masked max / argmax, blocked over rows so that a block's buffers stay below 1 GiB.  hipEvents around one
call, median (min .. max) of `--reps` after a warm-up call of each.  The composition is the yardstick; there is no
speed gate.  The two agree on the picks wherever fp32 rounding leaves no near-tie (reported, not asserted: the
composition's dot products are rocBLAS's, not the kernel's chain).

(ii) Quality.  A model trained here on synthetic ml-20m for a few epochs (as tools/foldin_probe.py trains its own);
the top 10 from a pool of 100 for 10,000 users at lam = 1.0, 0.7, 0.5: mean intra-list similarity (cosine) and the
mean relevance retained (the picks' scores above the pool's lowest, summed, over the same sum for the 10 best).

Writes profiles/diversify_probe.txt.
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr import engine as eng  # noqa: E402
from revisit_bpr.datasets import synthetic  # noqa: E402
from revisit_bpr.diversify import diversify, intra_list_similarity, recommend_diverse  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-study", action="store_true")
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--scale", type=float, default=0.25, help="fraction of ml-20m's users and actions the study trains on")
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "diversify_probe.txt"))
opt = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composition(Q, ci, cs, k, lam, metric):
    """greedy MMR in plain torch, scale = none, distinct valid ids: (items, scores)"""
    n, C = ci.shape
    d = Q.shape[1]
    out_i = torch.empty((n, k), dtype=torch.int32, device=dev)
    out_s = torch.empty((n, k), dtype=torch.float32, device=dev)
    step = max(1, (1 << 30) // (4 * C * max(C, d)))
    ninf = torch.tensor(float("-inf"), device=dev)
    for lo in range(0, n, step):
        ids, rel = ci[lo:lo + step].long(), cs[lo:lo + step]
        X = Q[ids]
        if metric == "cosine":
            X = X / X.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        S = torch.bmm(X, X.transpose(1, 2))
        m = torch.zeros_like(rel)
        left = torch.ones_like(rel, dtype=torch.bool)
        for t in range(k):
            v = torch.where(left, lam * rel - (1 - lam) * m, ninf)
            best = v.argmax(1, keepdim=True)
            out_i[lo:lo + step, t] = ids.gather(1, best).squeeze(1).int()
            out_s[lo:lo + step, t] = rel.gather(1, best).squeeze(1)
            left.scatter_(1, best, False)
            sim = S.gather(2, best.unsqueeze(1).expand(-1, C, 1)).squeeze(2)
            m = sim if t == 0 else torch.maximum(m, sim)
    return out_i, out_s


def distinct_pools(n, I, C, g):
    """[n, C] int32: every row C distinct ids of 1 .. I-1, uniformly (the C largest of I-1 uniform draws, by blocks)"""
    return torch.cat([torch.rand(min(1024, n - lo), I - 1, device=dev, generator=g).topk(C, dim=1).indices.int() + 1
                      for lo in range(0, n, 1024)])


def timing():
    say(f"(i) one call, lam 0.7, scale none; ms: median (min .. max) of {opt.reps}, fused and composition alternating")
    say(f"{'shape':22s} {'metric':>6s} {'n':>6s} {'C':>4s} {'k':>4s} | {'fused ms':>28s} | {'composition ms':>30s} | "
        f"{'comp / fused':>12s} | {'rows equal':>10s}")
    for name, I, d in (("ML-20M I=20109 d=128", 20_109, 128), ("MSD I=41140 d=256", 41_140, 256)):
        g = torch.Generator(device=dev).manual_seed(1)
        Q = torch.randn(I, d, device=dev, generator=g) * 0.1
        for metric in ("cosine", "dot"):
            for n in (1, 256, 10_000):
                for C, k in ((32, 10), (100, 10), (128, 20), (128, 128)):
                    ci = distinct_pools(n, I, C, g)
                    cs = torch.randn(n, C, device=dev, generator=g)
                    fused = lambda: diversify(Q, ci, cs, k, lam=0.7, metric=metric)  # noqa: E731
                    comp = lambda: composition(Q, ci, cs, k, 0.7, metric)  # noqa: E731
                    a, b = fused(), comp()
                    torch.cuda.synchronize()
                    equal = float((a[0] == b[0]).all(1).float().mean())
                    tf, tc = [], []
                    for _ in range(opt.reps):
                        tf.append(timed(fused))
                        tc.append(timed(comp))
                    tf.sort()
                    tc.sort()
                    mf, mc = tf[len(tf) // 2], tc[len(tc) // 2]
                    say(f"{name:22s} {metric:>6s} {n:6d} {C:4d} {k:4d} | {mf:10.3f} ({tf[0]:7.3f} .. {tf[-1]:7.3f}) | "
                        f"{mc:10.3f} ({tc[0]:8.3f} .. {tc[-1]:8.3f}) | {mc / mf:12.2f} | {equal:10.4f}")
                    del ci, cs, a, b
        del Q


def study():
    data = synthetic.generate_named("ml-20m", scale=opt.scale, seed=5)
    U, I, d = data.num_users, data.num_items, 128
    say()
    say(f"(ii) synthetic ml-20m x {opt.scale} ({U} users, {I} items, {data.nnz} actions), MF d = {d}, {opt.epochs} "
        f"epochs of the stream trainer (SGD lr 0.05, uniform negatives); top 10 of a pool of 100, cosine, minmax, "
        f"seen items left out")
    g = torch.Generator(device=dev).manual_seed(7)
    P = torch.randn(U, d, device=dev, generator=g) * 0.1
    Q = torch.randn(I, d, device=dev, generator=g) * 0.1
    P[0] = 0
    Q[0] = 0
    indptr, indices = torch.from_numpy(data.indptr).to(dev), torch.from_numpy(data.indices).to(dev)
    users, items = torch.from_numpy(data.users).to(dev), torch.from_numpy(data.items).to(dev)
    e = eng.Engine(P, Q)
    e.set_reg(0.001, 0.001, 0.001)
    e.set_optimizer(eng.OPT_SGD, lr=0.05)
    e.bind_seen_csr(indptr, indices)
    e.set_stream_opts(True, 0)
    n = users.numel()
    for ep in range(opt.epochs):
        pu, pi = e.plan_epoch(users, items, n, seed=7 + ep)
        e.train_stream(pu, pi, sampler=eng.NEG_UNIFORM, seed=7, offset=ep * n)
    e.hot_fold()
    torch.cuda.synchronize()
    e.close()
    who = torch.from_numpy(np.random.default_rng(3).choice(np.arange(1, U), min(10_000, U - 1), replace=False)
                           .astype(np.int32)).to(dev)
    from revisit_bpr.recommend import recommend

    pool_i, pool_s = recommend(P, Q, None, who, 100, indptr, indices)
    lo = torch.where(pool_i >= 0, pool_s, torch.tensor(float("inf"), device=dev)).min(1, keepdim=True).values
    base = None
    say(f"{'lam':>5s} | {'mean intra-list similarity':>26s} | {'relevance retained':>18s} | {'lists changed':>13s}")
    for lam in (1.0, 0.7, 0.5):
        it, sc = diversify(Q, pool_i, pool_s, 10, lam=lam, metric="cosine", scale="minmax")
        rd = recommend_diverse(P, Q, None, who, 10, pool=100, lam=lam, seen_indptr=indptr, seen_indices=indices)
        assert torch.equal(rd[0], it)
        base = (it, sc) if base is None else base
        ils = float(intra_list_similarity(Q, it).mean())
        kept = float(((sc - lo).sum(1) / (base[1] - lo).sum(1)).mean())  # of the 10 best's relevance above the pool's floor
        changed = float((it != base[0]).any(1).float().mean())
        say(f"{lam:5.2f} | {ils:26.4f} | {kept:18.4f} | {changed:13.4f}")

if not opt.skip_timing:
    timing()
if not opt.skip_study:
    study()
Path(opt.out).write_text("\n".join(lines) + "\n")
