#!/usr/bin/env python
"""What dynamic negative sampling costs and what it buys on an MI355X, beside the two samplers the engine had.

At the ML-20M shape (`synthetic.generate_named("ml-20m")`: 136,677 users, 20,108 items, ~9.7 M interactions, 10,000
evaluation users; d = 128, plain SGD at lr 0.001, reg as bench.py's ml-20m workload) a `fast.StreamTrainer` runs
`--epochs` epochs per sampler from the same initial model:

  uniform            sampler="uniform"
  adaptive (timed)   sampler="adaptive" with bench.py's SCHEDULE (refresh_lag 1, masked sort, LDS tier by the budget)
  dynamic M          sampler="dynamic", candidates M = 2, 4, 8, 16

The launch size is the schedule's (`resolve_schedule`: one refresh period, the same for every sampler).  Recorded:
  * triples/s of k_stream alone, from the library's hipEvents around each launch (`Engine.timing_enable`): after one
    warm-up epoch, five measurements of four launches each in the second epoch — median and range;
  * nDCG@100 and Recall@20 of the evaluation users after the last epoch (`evaluation.evaluate`).
Records, not gates.

Usage: python tools/dynamic_probe.py [--epochs 3] [--out profiles/dynamic_probe.txt]"""
import argparse
import statistics
import sys
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
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--lr", type=float, default=0.001)
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "dynamic_probe.txt"))
opt = ap.parse_args()
assert opt.epochs >= 2, "one warm-up epoch, then the timed one"
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


data = synthetic.generate_named("ml-20m", eval_users=10_000, seed=opt.seed)
t = {k: torch.from_numpy(getattr(data, k)).to(dev)
     for k in ("users", "items", "indptr", "indices", "eval_users", "eval_indptr", "eval_items")}
CONFIGS = [("uniform", dict(sampler="uniform")),
           ("adaptive (timed)", dict(sampler="adaptive", adaptive_p=0.01, refresh_lag=1.0, refresh_cus=-1))]
CONFIGS += [(f"dynamic M={m}", dict(sampler="dynamic", candidates=m)) for m in (2, 4, 8, 16)]

say(f"dynamic_probe: {torch.cuda.get_device_name(0)}; ml-20m shape U={data.num_users} I={data.num_items} "
    f"nnz={data.nnz} d={opt.dim} lr={opt.lr} epochs={opt.epochs}")
say(f"{'sampler':<18} {'launch':>8} {'ms/launch (median, min..max of 5)':>36} {'M triples/s':>12} {'x uniform':>10} "
    f"{'ndcg@100':>9} {'recall@20':>10} {'loss':>8}")
base_ms = None
for name, kw in CONFIGS:
    torch.manual_seed(opt.seed)
    model = BPR(fuse_forward=True,
                logits_model=MF(torch.nn.Embedding(data.num_users, opt.dim, padding_idx=0),
                                torch.nn.Embedding(data.num_items, opt.dim, padding_idx=0)),
                reg_alphas={"user": 0.0016, "item": 0.0001, "neg": 0.00375}).to(dev)
    tr = StreamTrainer(model, t["users"], t["items"], t["indptr"], t["indices"], lr=opt.lr, batch_size=256,
                       seed=opt.seed, **kw)
    e = tr.engine
    stats = tr.train_epoch()  # warm-up (and the first epoch of the curve)
    ms = []
    for _ in range(5):  # the second epoch: five measurements of four full launches each
        e.timing_enable(True)
        tr.train_chunks(4)
        torch.cuda.synchronize()
        avg, launches = e.timing_read()
        e.timing_enable(False)
        assert launches >= 4, launches
        ms.append(avg)
    stats = tr.train_chunks(10 ** 9)  # the rest of the second epoch
    for _ in range(opt.epochs - 2):
        stats = tr.train_epoch()
    torch.cuda.synchronize()
    model.eval()
    f = model.logits_model.get_features()
    res = evaluate(f["user"].detach(), f["item"].detach(), f["item_bias"], t["eval_users"], t["eval_indptr"],
                   t["eval_items"], t["indptr"], t["indices"], {"ndcg@100": NDCG(topk=100), "recall@20": Recall(topk=20)})
    med = statistics.median(ms)
    base_ms = med if base_ms is None else base_ms
    say(f"{name:<18} {tr.chunk:>8} {med:>14.4f} ({min(ms):.4f} .. {max(ms):.4f})      {tr.chunk / med / 1e3:>12.1f} "
        f"{med / base_ms:>10.2f} {res['ndcg@100']:>9.4f} {res['recall@20']:>10.4f} {stats['loss']:>8.4f}")
    del tr, model
    torch.cuda.empty_cache()
say("x uniform: the kernel's time per launch over the uniform kernel's.  adaptive: the k_stream launch alone — its "
    "snapshot sort runs beside it on masked CUs and is not in this figure.")
Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
Path(opt.out).write_text("\n".join(lines) + "\n")
