#!/usr/bin/env python
"""Two questions about fold-in (`revisit_bpr.foldin.fold_in`, csrc/bpr_foldin.hip), answered by measurement only.

(i) What does one call cost?  10,000 held-out users against a trained-scale item table at the ML-20M shape
(I = 20,109, d = 128; row lengths log-normal, median 37, tail in the thousands) for 5 and 20 epochs, and at the MSD
shape (I = 41,140, d = 256, median 30), sampled negatives, rows handed out longest first (`balance`) and in list
order.  hipEvents around one call (it includes the wrapper's argsort and its one host read), median and range of 5
runs after a warm-up.

(ii) Strong generalisation on `synthetic.generate_latent`: train on all users but 10 %, fold those in from their
training-side histories, and report `evaluate_topk` nDCG@100 on their held-out items beside the same users trained
jointly with everybody else (and beside untrained rows, the floor).

`--sampler adaptive` answers both for adaptive negatives (`fold_in(sampler="adaptive")`, csrc/bpr_foldin_adaptive.hip):
(i) on the same two shapes at 5 epochs, list order: the uniform kernel beside the adaptive one with its per-group LDS
bitmap and with the CSR search forced, snapshot built once outside the timed call, and the ratio adaptive / uniform
per triple; (ii) the same study with adaptive fold-in at `adaptive_p` 0.01 and `--study-p`, beside the uniform rows.
The prefetch depth is a compile-time constant of the library: point BPR_LIB_PATH at a build made with
-DBPR_FOLDIN_ADAPTIVE_PF=N and pass --label to name it in the output.

`--sampler dynamic|warp [--candidates N]` answers (i) for the scored negatives (`fold_in(sampler="dynamic" | "warp")`,
csrc/bpr_foldin_scored.hip): the same two shapes at 5 epochs, list order, the uniform kernel in the same process beside
the scored one with its per-group LDS bitmap and with the CSR search forced, at N = 4 and 10 candidates (or
`--candidates` alone), and the ratio to the uniform leg; under WARP also the shares of the call's draws that ended at
tries = 1 and that were skipped.  (ii) is a study of its own, the same under either of the two (run it once:
--skip-study on the other): does folding in with the sampler the table was trained with rank better?  On
`synthetic.generate_structured` at the ML-20M shape, d = 128, one table is trained by `StreamTrainer(sampler="warp")`
at lr 0.001 and one with uniform negatives under BPR's loss at lr 0.01 (each objective's better rate of DESIGN §4.17),
5 epochs, each with everybody and without 400 of the evaluation users; those are folded into the table trained without
them with uniform, dynamic and WARP steps at 5 / 20 / 60 epochs, each step at the learning rate of its own loss, and
their nDCG@100 stands beside the jointly trained and the untrained rows.

Usage: python tools/foldin_probe.py [--reps 5] [--skip-study] [--skip-timing] [--sampler uniform|adaptive|dynamic|warp]
                                    [--candidates N] [--study-p 0.05] [--scale 1.0] [--label TEXT] [--append]
                                    [--out profiles/foldin_probe.txt]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "revisit-bpr_amd")]
from revisit_bpr import engine as eng  # noqa: E402
from revisit_bpr.datasets import synthetic  # noqa: E402
from revisit_bpr.evaluation import evaluate_topk  # noqa: E402
from revisit_bpr.foldin import fold_in, snapshot_of  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-study", action="store_true")
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--sampler", choices=("uniform", "adaptive", "dynamic", "warp"), default="uniform")
ap.add_argument("--candidates", type=int, default=0, help="scored samplers: time this N alone (default: 4 and 10)")
ap.add_argument("--study-p", type=float, default=0.05, help="second adaptive_p of the study (beside 0.01)")
ap.add_argument("--scale", type=float, default=1.0,
                help="scored samplers' study: users and interactions of its data set times this (a quick look)")
ap.add_argument("--label", type=str, default="")
ap.add_argument("--append", action="store_true")
ap.add_argument("--out", type=str, default=None)
opt = ap.parse_args()
if opt.out is None:
    opt.out = str(ROOT / "profiles" / {"uniform": "foldin_probe.txt", "adaptive": "foldin_probe_adaptive.txt"}.get(
        opt.sampler, "foldin_probe_scored.txt"))
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def histories(n, I, median, sigma, seed):
    """n sorted rows of distinct items in [1, I), lengths log-normal(median, sigma) clipped to [1, I // 3]"""
    rng = np.random.default_rng(seed)
    lens = np.clip(np.round(median * np.exp(sigma * rng.standard_normal(n))), 1, I // 3).astype(np.int64)
    rows = [np.sort(rng.choice(I - 1, size=int(k), replace=False) + 1) for k in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return torch.from_numpy(indptr).to(dev), torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev), lens


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timing():
    say(f"(i) one fold_in call, sampled negatives, lr 0.05, reg_user 0.01; ms: median  min .. max of {opt.reps}")
    say(f"{'shape':30s} {'users':>6s} {'nnz':>9s} {'longest':>7s} {'epochs':>6s} {'balance':>7s} | "
        f"{'ms':>26s} | {'M triples/s':>11s}")
    for name, I, d, median, sigma, epoch_list in (("ML-20M I=20109 d=128", 20_109, 128, 37.0, 1.4, (5, 20)),
                                                  ("MSD I=41140 d=256", 41_140, 256, 30.0, 1.0, (5,))):
        g = torch.Generator(device=dev).manual_seed(1)
        Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
        b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
        indptr, items, lens = histories(10_000, I, median, sigma, seed=2)
        nnz = int(lens.sum())
        for epochs in epoch_list:
            res = {}
            for balance in (True, False):
                call = lambda: fold_in(Q, b, indptr, items, epochs=epochs, lr=0.05, reg_user=0.01, init_std=0.01,  # noqa: E731
                                       seed=3, balance=balance)
                res[balance] = call()
                ms = sorted(timed(call) for _ in range(opt.reps))
                say(f"{name:30s} {10_000:6d} {nnz:9d} {int(lens.max()):7d} {epochs:6d} {str(balance):>7s} | "
                    f"{ms[len(ms) // 2]:10.3f}  {ms[0]:6.3f} .. {ms[-1]:6.3f} | {epochs * nnz / ms[len(ms) // 2] / 1e3:11.1f}")
            assert torch.equal(res[True], res[False])
        del Q, b, indptr, items


def timing_adaptive():
    say(f"(i) one fold_in call, 5 epochs, lr 0.05, reg_user 0.01, list order (balance off); adaptive_p 0.01, snapshot "
        f"built outside the timed call; ms: median  min .. max of {opt.reps}  [{opt.label or 'library as built'}]")
    say(f"{'shape':24s} {'nnz':>9s} {'negatives':>18s} | {'ms':>28s} | {'M triples/s':>11s} | {'x uniform':>9s}")
    for name, I, d, median, sigma in (("ML-20M I=20109 d=128", 20_109, 128, 37.0, 1.4),
                                      ("MSD I=41140 d=256", 41_140, 256, 30.0, 1.0)):
        g = torch.Generator(device=dev).manual_seed(1)
        Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
        b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
        indptr, items, lens = histories(10_000, I, median, sigma, seed=2)
        nnz, epochs = int(lens.sum()), 5
        snap = snapshot_of(Q)  # (built once; the timed call copies `order` into its padded buffer, 4 d I bytes)
        kw = dict(epochs=epochs, lr=0.05, reg_user=0.01, init_std=0.01, seed=3, balance=False)
        legs = (("uniform", dict()), ("adaptive, bitmap", dict(sampler="adaptive", snapshot=snap, _seen_mode=2)),
                ("adaptive, CSR", dict(sampler="adaptive", snapshot=snap, _seen_mode=1)))
        base, outs = None, {}
        for leg, extra in legs:
            call = lambda: fold_in(Q, b, indptr, items, **kw, **extra)  # noqa: E731
            outs[leg] = call()
            ms = sorted(timed(call) for _ in range(opt.reps))
            med = ms[len(ms) // 2]
            base = med if base is None else base
            say(f"{name:24s} {nnz:9d} {leg:>18s} | {med:10.3f}  {ms[0]:7.3f} .. {ms[-1]:7.3f} | "
                f"{epochs * nnz / med / 1e3:11.1f} | {med / base:9.2f}")
        assert torch.equal(outs["adaptive, bitmap"], outs["adaptive, CSR"])
        del Q, b, indptr, items, snap


def timing_scored():
    say(f"(i) one fold_in call, 5 epochs, lr 0.05, reg_user 0.01, list order (balance off); sampler {opt.sampler}, "
        f"margin 1.0; ms: median  min .. max of {opt.reps}  [{opt.label or 'library as built'}]")
    say(f"{'shape':24s} {'nnz':>9s} {'negatives':>22s} | {'ms':>28s} | {'M triples/s':>11s} | {'x uniform':>9s}"
        + (f" | {'tries = 1':>9s} {'skipped':>8s}   (shares of the call's 5 x nnz draws)" if opt.sampler == "warp"
           else ""))
    for name, I, d, median, sigma in (("ML-20M I=20109 d=128", 20_109, 128, 37.0, 1.4),
                                      ("MSD I=41140 d=256", 41_140, 256, 30.0, 1.0)):
        g = torch.Generator(device=dev).manual_seed(1)
        Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
        b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
        indptr, items, lens = histories(10_000, I, median, sigma, seed=2)
        nnz, epochs = int(lens.sum()), 5
        kw = dict(epochs=epochs, lr=0.05, reg_user=0.01, init_std=0.01, seed=3, balance=False)
        legs = [("uniform", dict())]
        for N in ((opt.candidates,) if opt.candidates else (4, 10)):
            scored = dict(sampler=opt.sampler, candidates=N, max_sampled=N, margin=1.0)
            legs += [(f"{opt.sampler} N={N}, bitmap", dict(scored, _seen_mode=2)),
                     (f"{opt.sampler} N={N}, CSR", dict(scored, _seen_mode=1))]
        base, outs = None, {}
        for leg, extra in legs:
            call = lambda **more: fold_in(Q, b, indptr, items, **kw, **extra, **more)  # noqa: E731
            draws = ""
            if "sampler" in extra:  # the warm-up call also says what the draws of this leg were
                outs[leg], neg, tries = call(return_neg=True, return_draws=True)
                if opt.sampler == "warp":
                    draws = (f" | {(tries == 1).float().mean().item():9.4f} {(neg < 0).float().mean().item():8.4f}")
                del neg, tries
            else:
                outs[leg] = call()
            ms = sorted(timed(call) for _ in range(opt.reps))
            med = ms[len(ms) // 2]
            base = med if base is None else base
            say(f"{name:24s} {nnz:9d} {leg:>22s} | {med:10.3f}  {ms[0]:7.3f} .. {ms[-1]:7.3f} | "
                f"{epochs * nnz / med / 1e3:11.1f} | {med / base:9.2f}{draws}")
        for (la, _), (lb, _) in zip(legs[1::2], legs[2::2]):
            assert torch.equal(outs[la], outs[lb])
        del Q, b, indptr, items


def train(users, items, indptr, indices, U, I, d, epochs, lr, reg, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    P = torch.randn(U, d, device=dev, generator=g) * 0.1
    Q = torch.randn(I, d, device=dev, generator=g) * 0.1
    P[0] = 0
    Q[0] = 0
    e = eng.Engine(P, Q)
    e.set_reg(reg, reg, reg)
    e.set_optimizer(eng.OPT_SGD, lr=lr)
    e.bind_seen_csr(indptr, indices)
    e.set_stream_opts(True, 0)
    n = users.numel()
    for ep in range(epochs):
        pu, pi = e.plan_epoch(users, items, n, seed=seed + ep)
        e.train_stream(pu, pi, sampler=eng.NEG_UNIFORM, seed=seed, offset=ep * n)
    e.hot_fold()
    torch.cuda.synchronize()
    e.close()
    return P, Q


def study():
    U0, I0, d, epochs, lr, reg = 4000, 1500, 32, 60, 0.05, 0.002
    data = synthetic.generate_latent(U0, I0, 240_000, factors=16, seed=5)
    rng = np.random.default_rng(6)
    held = np.sort(rng.choice(np.arange(1, data.num_users), size=U0 // 10, replace=False))
    is_held = np.zeros(data.num_users, bool)
    is_held[held] = True
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    # jointly: everybody trains
    Pj, Qj = train(t(data.users), t(data.items), t(data.indptr), t(data.indices), data.num_users, data.num_items, d,
                   epochs, lr, reg, seed=7)
    # without the held-out users: their triples leave the training set, their CSR rows are empty
    keep = ~is_held[data.users]
    cnt = np.diff(data.indptr) * ~is_held
    Pw, Qw = train(t(data.users[keep]), t(data.items[keep]), t(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)),
                   t(data.indices[keep]), data.num_users, data.num_items, d, epochs, lr, reg, seed=7)
    # the held-out users as a list of their own: histories (seen CSR) and targets (eval CSR), re-based
    h_cnt = np.diff(data.indptr)[held]
    h_indptr = np.concatenate([[0], np.cumsum(h_cnt)]).astype(np.int64)
    h_items = np.concatenate([data.indices[data.indptr[u]:data.indptr[u + 1]] for u in held]).astype(np.int32)
    pos = np.searchsorted(data.eval_users, held)
    assert np.array_equal(data.eval_users[pos], held)
    e_cnt = np.diff(data.eval_indptr)[pos]
    e_indptr = np.concatenate([[0], np.cumsum(e_cnt)]).astype(np.int64)
    e_items = np.concatenate([data.eval_items[data.eval_indptr[k]:data.eval_indptr[k + 1]] for k in pos]).astype(np.int32)
    rows = torch.arange(len(held), dtype=torch.int32, device=dev)

    def ndcg(P, Q):
        return evaluate_topk(P, Q, None, rows, t(e_indptr), t(e_items), t(h_indptr), t(h_items), ks=(100,))["ndcg@100"]

    say()
    say(f"(ii) generate_latent({U0} users, {I0} items, 240,000 actions, 16 factors), d = {d}, SGD lr {lr}, reg {reg}, "
        f"{epochs} epochs of uniform-negative STREAM training; {len(held)} users held out; nDCG@100 of those users on "
        f"their held-out items")
    say(f"  trained jointly with everybody                      {ndcg(Pj[t(held).long()], Qj):.4f}")
    for fe in (5, 20, 60):
        Pn = fold_in(Qw, None, t(h_indptr), t(h_items), epochs=fe, lr=lr, reg_user=reg, init_std=0.1, seed=8)
        say(f"  folded in against the table trained without them, {fe:2d} epochs   {ndcg(Pn, Qw):.4f}")
    if opt.sampler == "adaptive":
        snap = snapshot_of(Qw)
        for ap_ in (0.01, opt.study_p):
            for fe in (5, 20, 60):
                Pn = fold_in(Qw, None, t(h_indptr), t(h_items), epochs=fe, lr=lr, reg_user=reg, init_std=0.1, seed=8,
                             sampler="adaptive", adaptive_p=ap_, snapshot=snap)
                say(f"  folded in with ADAPTIVE negatives, adaptive_p {ap_:<5g} {fe:2d} epochs   {ndcg(Pn, Qw):.4f}")
    say(f"  untrained rows (N(0, 0.1^2)) against that table     "
        f"{ndcg(torch.randn(len(held), d, device=dev) * 0.1, Qw):.4f}")


def study_scored():
    """Fold in with the sampler the table was trained with — does it rank better?  One table trained under WARP and one
    under BPR with uniform negatives, each at its better learning rate of DESIGN §4.17, each twice: with everybody and
    without the held-out users.  The same for `--sampler dynamic` and `--sampler warp`."""
    from revisit_bpr.fast import StreamTrainer
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF

    d, epochs, held_n, seed = 128, 5, 400, 13
    M, N = opt.candidates or 4, opt.candidates or 10
    reg = {"user": 0.0016, "item": 0.0001, "neg": 0.00375}  # bench.py's ml-20m workload, as tools/warp_probe.py
    std = 1.0 / (d * 12 ** 0.5)  # the std of MF's initial rows, U[-0.5, 0.5) / d
    users, items, actions, _, _ = synthetic.SHAPES["ml-20m"]
    users, actions = max(held_n + 16, int(users * opt.scale)), max(64, int(actions * opt.scale))
    data = synthetic.generate_structured(users, items, actions, seed=seed, eval_users=min(10_000, users))
    rng = np.random.default_rng(6)
    held = np.sort(rng.choice(data.eval_users.astype(np.int64), size=held_n, replace=False))
    is_held = np.zeros(data.num_users, bool)
    is_held[held] = True
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    # without the held-out users: their triples leave the training set, their CSR rows are empty
    keep = ~is_held[data.users]
    cnt = np.diff(data.indptr) * ~is_held
    everybody = (t(data.users), t(data.items), t(data.indptr), t(data.indices))
    without = (t(data.users[keep]), t(data.items[keep]), t(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)),
               t(data.indices[keep]))
    # the held-out users as a list of their own: histories (seen CSR) and targets (eval CSR), re-based
    h_cnt = np.diff(data.indptr)[held]
    h_indptr = t(np.concatenate([[0], np.cumsum(h_cnt)]).astype(np.int64))
    h_items = t(np.concatenate([data.indices[data.indptr[u]:data.indptr[u + 1]] for u in held]).astype(np.int32))
    pos = np.searchsorted(data.eval_users, held)
    assert np.array_equal(data.eval_users[pos], held)
    e_cnt = np.diff(data.eval_indptr)[pos]
    e_indptr = t(np.concatenate([[0], np.cumsum(e_cnt)]).astype(np.int64))
    e_items = t(np.concatenate([data.eval_items[data.eval_indptr[k]:data.eval_indptr[k + 1]] for k in pos])
                .astype(np.int32))
    rows = torch.arange(held_n, dtype=torch.int32, device=dev)

    def train(tensors, lr, kw):
        torch.manual_seed(seed)
        model = BPR(fuse_forward=True,
                    logits_model=MF(torch.nn.Embedding(data.num_users, d, padding_idx=0),
                                    torch.nn.Embedding(data.num_items, d, padding_idx=0)), reg_alphas=reg).to(dev)
        tr = StreamTrainer(model, *tensors, lr=lr, batch_size=256, seed=seed, **kw)
        for _ in range(epochs):
            tr.train_epoch()
        torch.cuda.synchronize()
        model.eval()
        f = model.logits_model.get_features()
        P, Q = f["user"].detach().clone(), f["item"].detach().clone()
        del tr, model
        torch.cuda.empty_cache()
        return P, Q

    def ndcg(P, Q):
        return evaluate_topk(P, Q, None, rows, e_indptr, e_items, h_indptr, h_items, ks=(100,))["ndcg@100"]

    bpr_lr, warp_lr = 0.01, 0.001
    steps = ((f"uniform negatives, BPR's step, lr {bpr_lr}", bpr_lr, dict()),
             (f"dynamic M={M}, BPR's step, lr {bpr_lr}", bpr_lr, dict(sampler="dynamic", candidates=M)),
             (f"WARP N={N} margin 1, lr {warp_lr}", warp_lr, dict(sampler="warp", max_sampled=N, margin=1.0)))
    say()
    say(f"(ii) generate_structured({users} users, {items} items, {actions} interactions; rank 16, skew 1, temperature 1), "
        f"d = {d}, SGD, reg {reg['user']} / {reg['item']} / {reg['neg']}, {epochs} epochs of STREAM training; {held_n} "
        f"of the evaluation users held out ({int(h_cnt.sum())} history entries, {int(e_cnt.sum())} targets); nDCG@100 "
        f"of those users on their targets.  Fold-in: reg_user {reg['user']}, rows from N(0, {std:.5f}^2), each step "
        f"at the learning rate its loss was trained with; 'skipped': share of the 60-epoch call's triples WARP skipped")
    for title, lr, kw in ((f"table trained under WARP (max_sampled {N}, margin 1), lr {warp_lr}", warp_lr,
                           dict(sampler="warp", max_sampled=N, margin=1.0)),
                          (f"table trained under BPR with uniform negatives, lr {bpr_lr}", bpr_lr,
                           dict(sampler="uniform"))):
        Pj, Qj = train(everybody, lr, kw)
        joint = ndcg(Pj[t(held)], Qj)
        del Pj, Qj
        _, Qw = train(without, lr, kw)
        g = torch.Generator(device=dev).manual_seed(8)
        floor = ndcg(torch.randn(held_n, d, device=dev, generator=g) * std, Qw)
        say()
        say(f"{title}")
        say(f"  {'trained jointly with everybody':44s} {joint:8.4f}")
        say(f"  {'untrained rows against the table without them':44s} {floor:8.4f}")
        say(f"  {'folded in against the table without them':44s} {'5 epochs':>8s} {'20':>8s} {'60':>8s} {'skipped':>8s}")
        for leg, flr, extra in steps:
            vals, skipped = [], "-"
            for fe in (5, 20, 60):
                out = fold_in(Qw, None, h_indptr, h_items, epochs=fe, lr=flr, reg_user=reg["user"], init_std=std,
                              seed=8, return_neg=True, **extra)
                vals.append(ndcg(out[0], Qw))
                if extra.get("sampler") == "warp":
                    skipped = f"{(out[1] < 0).float().mean().item():.4f}"
            say(f"  {leg:44s} " + " ".join(f"{v:8.4f}" for v in vals) + f" {skipped:>8s}")
        del Qw


say(f"device {torch.cuda.get_device_name(0)}")
if not opt.skip_timing:
    {"uniform": timing, "adaptive": timing_adaptive}.get(opt.sampler, timing_scored)()
if not opt.skip_study:
    (study_scored if opt.sampler in ("dynamic", "warp") else study)()
Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
with open(opt.out, "a" if opt.append else "w") as fh:
    fh.write("\n".join(lines) + "\n")
