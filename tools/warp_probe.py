#!/usr/bin/env python
"""What the WARP objective costs and what it buys on an MI355X, beside uniform and dynamic negatives under BPR's loss.

Two data sets of the ML-20M shape (136,677 users, 20,108 items, ~9.7 M interactions, 10,000 evaluation users):
`synthetic.generate_named("ml-20m")`, whose items are drawn by popularity alone, and `synthetic.generate_structured` of
the same shape, whose users have factors of their own.  d = 128, plain SGD, reg as bench.py's ml-20m workload.  A
`fast.StreamTrainer` runs `--epochs` epochs per leg from the same initial model:

  uniform        sampler="uniform"
  dynamic M      sampler="dynamic", candidates M = 4, 10
  warp N         sampler="warp", max_sampled N = 1, 4, 10, 32, margin 1

Recorded:
  * k_stream alone, from the library's hipEvents around each launch (`Engine.timing_enable`), on the ML-20M shape at
    the first learning rate: after one warm-up epoch, five measurements of four launches each in the second epoch —
    median and range of ms per launch, triples/s (triples LOOKED AT: a skipped triple costs its candidates), and the
    ratio to the uniform leg of the same run;
  * the share of triples WARP skipped in the first and in the last epoch;
  * nDCG@100 and Recall@20 of the evaluation users after the last epoch (`evaluation.evaluate`), per data set and
    learning rate.
Records, not gates.

Usage: python tools/warp_probe.py [--epochs 5] [--lrs 0.001,0.01] [--out profiles/warp_probe.txt]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr.datasets import synthetic  # noqa: E402
from revisit_bpr.evaluation import evaluate  # noqa: E402
from revisit_bpr.fast import StreamTrainer  # noqa: E402
from revisit_bpr.metrics import NDCG, Recall  # noqa: E402
from revisit_bpr.models import BPR  # noqa: E402
from revisit_bpr.models.bpr import MF  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=5)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--lrs", type=str, default="0.001,0.01")
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--scale", type=float, default=1.0, help="users and interactions of both sets times this (a quick look)")
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "warp_probe.txt"))
opt = ap.parse_args()
assert opt.epochs >= 2, "one warm-up epoch, then the timed one"
lrs = [float(x) for x in opt.lrs.split(",")]
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


CONFIGS = [("uniform", dict(sampler="uniform"))]
CONFIGS += [(f"dynamic M={m}", dict(sampler="dynamic", candidates=m)) for m in (4, 10)]
CONFIGS += [(f"warp N={n}", dict(sampler="warp", max_sampled=n, margin=1.0)) for n in (1, 4, 10, 32)]

users, items, actions, _, _ = synthetic.SHAPES["ml-20m"]
users, actions = max(16, int(users * opt.scale)), max(64, int(actions * opt.scale))
n_eval = min(10_000, users)
t0 = time.time()
SETS = [("ml-20m shape, items by popularity alone", synthetic.generate_named("ml-20m", eval_users=n_eval, seed=opt.seed,
                                                                             scale=opt.scale))]
t1 = time.time()
SETS.append(("ml-20m shape, generate_structured (rank 16, skew 1, temperature 1)",
             synthetic.generate_structured(users, items, actions, seed=opt.seed, eval_users=n_eval)))
say(f"warp_probe: {torch.cuda.get_device_name(0)}; d={opt.dim} epochs={opt.epochs} lrs={lrs}; data generated in "
    f"{t1 - t0:.0f} s + {time.time() - t1:.0f} s")


def run(data, t, lr, kw, timed):
    torch.manual_seed(opt.seed)
    model = BPR(fuse_forward=True,
                logits_model=MF(torch.nn.Embedding(data.num_users, opt.dim, padding_idx=0),
                                torch.nn.Embedding(data.num_items, opt.dim, padding_idx=0)),
                reg_alphas={"user": 0.0016, "item": 0.0001, "neg": 0.00375}).to(dev)
    tr = StreamTrainer(model, t["users"], t["items"], t["indptr"], t["indices"], lr=lr, batch_size=256,
                       seed=opt.seed, **kw)
    e = tr.engine
    first = tr.train_epoch()  # warm-up (and the first epoch of the curve)
    ms = []
    if timed:
        for _ in range(5):  # the second epoch: five measurements of four full launches each
            e.timing_enable(True)
            tr.train_chunks(4)
            torch.cuda.synchronize()
            avg, launches = e.timing_read()
            e.timing_enable(False)
            assert launches >= 4, launches
            ms.append(avg)
        last = tr.train_chunks(10 ** 9)  # the rest of the second epoch
    else:
        last = tr.train_epoch()
    for _ in range(opt.epochs - 2):
        last = tr.train_epoch()
    torch.cuda.synchronize()
    model.eval()
    f = model.logits_model.get_features()
    res = evaluate(f["user"].detach(), f["item"].detach(), f["item_bias"], t["eval_users"], t["eval_indptr"],
                   t["eval_items"], t["indptr"], t["indices"], {"ndcg@100": NDCG(topk=100), "recall@20": Recall(topk=20)})
    chunk = tr.chunk
    del tr, model
    torch.cuda.empty_cache()
    return ms, chunk, first, last, res


for si, (title, data) in enumerate(SETS):
    t = {k: torch.from_numpy(getattr(data, k)).to(dev)
         for k in ("users", "items", "indptr", "indices", "eval_users", "eval_indptr", "eval_items")}
    for li, lr in enumerate(lrs):
        timed = si == 0 and li == 0
        say()
        say(f"{title}: U={data.num_users} I={data.num_items} nnz={data.nnz} lr={lr}")
        head = f"{'leg':<14}"
        if timed:
            head += f" {'launch':>8} {'ms/launch (median, min..max of 5)':>36} {'M triples/s':>12} {'x uniform':>10}"
        say(head + f" {'skipped e1':>11} {'skipped last':>13} {'ndcg@100':>9} {'recall@20':>10} {'loss':>9}")
        base_ms = None
        for name, kw in CONFIGS:
            ms, chunk, first, last, res = run(data, t, lr, kw, timed)
            row = f"{name:<14}"
            if timed:
                med = statistics.median(ms)
                base_ms = med if base_ms is None else base_ms
                row += (f" {chunk:>8} {med:>14.4f} ({min(ms):.4f} .. {max(ms):.4f})      {chunk / med / 1e3:>12.1f} "
                        f"{med / base_ms:>10.2f}")
            warp = kw["sampler"] == "warp"
            # (the timed epoch is read in pieces: its last piece's count says nothing about the epoch)
            sk1 = f"{1 - first['triples'] / data.nnz:>11.4f}" if warp else f"{'-':>11}"
            skl = f"{1 - last['triples'] / data.nnz:>13.4f}" if warp and not (timed and opt.epochs == 2) else f"{'-':>13}"
            say(row + f" {sk1} {skl} {res['ndcg@100']:>9.4f} {res['recall@20']:>10.4f} {last['loss']:>9.4f}")
say()
say("x uniform: the kernel's time per launch over the uniform kernel's, same run.  triples/s counts every triple the "
    "launch looked at, skipped ones included.  loss: BPR's for uniform and dynamic, WARP's sum L (margin - x_i + x_k) "
    "over the stepped triples for warp — not comparable across the two.")
Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
Path(opt.out).write_text("\n".join(lines) + "\n")
