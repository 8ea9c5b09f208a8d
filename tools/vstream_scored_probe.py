#!/usr/bin/env python
"""What the scored samplers cost inside the batched STREAM launch on an MI355X, beside what the engine had before.

At the Yelp shape (`synthetic.generate_named("yelp")`: 252,616 users, 92,089 items, ~2.2 M interactions; d = 128, no
item_bias, virtual batches of 256, reg as bench.py's) one epoch of the shuffled stream runs under Adam and under Adagrad:

  uniform            bpr_train_stream_batched(NEG_UNIFORM): the launch the engine had, same shape   (baseline 1)
  per-batch loop     the documented workaround for dynamic negatives with a stateful optimizer: per virtual batch one
                     bpr_sample_dynamic(M = 4) and one bpr_train_stream_batched(NEG_GIVEN) launch    (baseline 2;
                     timed over --loop-batches batches — the whole epoch is 8,600 pairs of launches)
  dynamic M = 4      bpr_train_stream_batched_scored(NEG_DYNAMIC)
  WARP N = 10        bpr_train_stream_batched_scored(NEG_WARP, margin 1.0)

Both baselines run the kernels the parent commit ran: this change leaves every existing k_vstream / k_vflush
instantiation and the stand-alone sampler untouched (profiles/vstream_scored_resources.md).  Each leg starts from the
same tables, takes one untimed warm-up epoch and is then timed over --repeats epochs (wall clock around
torch.cuda.synchronize; median and range).  The run-to-run spread is what the repeats of the uniform leg show.
Recorded: M triples/s, the ratio to the uniform launch, WARP's skipped share in the last timed epoch.  Records, not
gates.

Usage: python tools/vstream_scored_probe.py [--repeats 5] [--out profiles/vstream_scored_probe.txt]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr import engine as eng  # noqa: E402
from revisit_bpr.datasets import synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--loop-batches", type=int, default=400)
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "vstream_scored_probe.txt"))
opt = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


data = synthetic.generate_named("yelp", seed=opt.seed)
t = {k: torch.from_numpy(getattr(data, k)).to(dev) for k in ("users", "items", "indptr", "indices")}
n, B, d = data.nnz, opt.batch, opt.dim
g = torch.Generator().manual_seed(opt.seed)
P0 = ((torch.rand(data.num_users, d, generator=g) - 0.5) / d * 8)
Q0 = ((torch.rand(data.num_items, d, generator=g) - 0.5) / d * 8)
P0[0] = 0
Q0[0] = 0
OPTS = {"adam": dict(kind=eng.OPT_ADAM, lr=0.002, betas=(0.1, 0.999)),
        "adagrad": dict(kind=eng.OPT_ADAGRAD, lr=0.05, eps=1e-10)}


def fresh(cfg):
    e = eng.Engine(P0.to(dev), Q0.to(dev))
    e.set_reg(0.0016, 0.0001, 0.00375)
    e.bind_seen_csr(t["indptr"], t["indices"])
    e.set_optimizer(**cfg)
    e.alloc_opt_state()
    e.set_dynamic(4)
    e.set_warp(10, 1.0)
    return e


def timed(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return count / (time.perf_counter() - t0) / 1e6


say(f"vstream_scored_probe: {torch.cuda.get_device_name(0)}; yelp shape U={data.num_users} I={data.num_items} nnz={n} "
    f"d={d} B={B}, no item_bias, max_inflight 0 (the chip full), {opt.repeats} timed epochs per leg after one warm-up")
say(f"{'optimizer':<9} {'leg':<18} {'M triples/s (median, min..max)':>34} {'x uniform':>10} {'skipped':>9}")
for oname, cfg in OPTS.items():
    base = None
    for leg in ("uniform", "per-batch loop", "dynamic M=4", "WARP N=10"):
        e = fresh(cfg)
        pu, pi = e.shuffle_epoch(t["users"], t["items"], seed=5)
        neg = torch.empty(n, dtype=torch.int32, device=dev)
        sc = torch.zeros(4, device=dev)
        drawn = [0]

        if leg == "uniform":
            def epoch():
                e.train_stream_batched(pu, pi, B, sampler=eng.NEG_UNIFORM, seed=3, offset=drawn[0], scalars=sc)
            count = n
        elif leg == "per-batch loop":
            count = min(opt.loop_batches * B, n)

            def epoch():
                for lo in range(0, count, B):
                    hi = min(lo + B, count)
                    nb = e.sample_dynamic(pu[lo:hi], 4, seed=3, offset=drawn[0] + lo)
                    e.train_stream_batched(pu[lo:hi], pi[lo:hi], B, sampler=eng.NEG_GIVEN, neg=nb, scalars=sc)
        else:
            kind = eng.NEG_DYNAMIC if leg.startswith("dynamic") else eng.NEG_WARP

            def epoch():
                e.train_stream_batched_scored(pu, pi, B, kind, neg=neg, seed=3, offset=drawn[0], scalars=sc)
            count = n
        epoch()  # warm-up
        drawn[0] += n
        rates, skipped = [], ""
        for _ in range(opt.repeats):
            sc.zero_()
            rates.append(timed(epoch, count))
            drawn[0] += n
            if leg.startswith("WARP"):
                skipped = f"{1.0 - float(sc[3]) / n:8.1%}"
        e.flush_lazy()
        assert bool(torch.isfinite(e.P).all()) and bool(torch.isfinite(e.Q).all())
        med = statistics.median(rates)
        base = med if leg == "uniform" else base
        say(f"{oname:<9} {leg:<18} {med:14.1f}  ({min(rates):7.1f} .. {max(rates):7.1f})   {med / base:9.2f}x {skipped:>9}")
say()
say("uniform and per-batch loop run kernels this change leaves as the parent commit built them.  The per-batch loop is")
say(f"timed over its first {opt.loop_batches} batches; the fused legs and the uniform launch over the whole epoch.")
say(f"skipped: WARP triples without a violator among N = 10, as a share of the LAST timed epoch — the model has trained")
say(f"for {opt.repeats + 1} epochs by then, and a trained model leaves fewer violators (more candidates viewed per triple).")
Path(opt.out).write_text("\n".join(lines) + "\n")
