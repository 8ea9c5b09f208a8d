#!/usr/bin/env python
"""Two questions about item fold-in (`revisit_bpr.foldin_items.fold_in_items`, csrc/bpr_foldin_items.hip), answered by
measurement only.

(i) What does one call cost?  2,000 new items against trained-scale tables at the ML-20M shape (U = 138,493,
I = 20,109, d = 128, seen rows of 144 items on average) and at the MSD shape (U = 571,355, I = 41,140, d = 256, 59 on
average), 5 epochs, sampled negatives, item bias.  The audiences follow an item-popularity skew: log-normal lengths
(median 40, sigma 2.0 / median 20, sigma 1.5: most new items have a few dozen users, a few have tens of thousands),
distinct users spread evenly over the table.  Rows handed out longest first (`balance`) and in list order.  hipEvents
around one call (it includes the wrapper's argsort and its host read), median and range of 5 runs after a warm-up.

(ii) Cold-start quality on `synthetic.generate_latent`: train without 10 % of the items (they leave the catalogue: no
positive and no negative ever touches them), fold them in from the training-side interactions with them, and report
nDCG@100 of the held-out interactions WITH THOSE ITEMS, ranked in the whole catalogue, beside the same items trained
jointly with everything else and beside untrained rows (the floor); and, second column, nDCG@100 of ALL held-out
interactions, which charges a new item for the warm targets it displaces.  Folded-in items get no updates in the
negative role; this table is how far that matters.

With `--neg-role auto` (or N) both questions are asked of the second role (`fold_in_items(neg_role=...)`,
csrc/bpr_foldin_items_roles.hip): (i) times the same two lists with R negative-role steps per row and epoch against
R = 0 through the single-role entry, alternating in one process, and reports microseconds per sequential step of the
longest row on both sides (the training interactions are the seen CSR's); (ii) adds the rows folded in with R to the
table, beside R = 0, at 5 / 20 / 60 epochs.  The output then goes to profiles/foldin_items_roles_probe.txt.

Usage: python tools/foldin_items_probe.py [--reps 5] [--skip-study] [--skip-timing] [--neg-role {0,auto,N}]
       [--out profiles/foldin_items_probe.txt]"""
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
from revisit_bpr.foldin_items import fold_in_items  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-study", action="store_true")
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--neg-role", type=str, default="0", help="0 (single role), auto, or a count per row and epoch")
ap.add_argument("--out", type=str, default=None)
opt = ap.parse_args()
NEG_ROLE = "auto" if opt.neg_role == "auto" else int(opt.neg_role)
if opt.out is None:
    opt.out = str(ROOT / "profiles" / ("foldin_items_roles_probe.txt" if NEG_ROLE != 0 else "foldin_items_probe.txt"))
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def strided_csr(cnt, n_ids, first, g):
    """CSR whose row r holds cnt[r] sorted, distinct ids in [first, n_ids): evenly strided from a per-row offset"""
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cnt, 0)])
    stride = torch.clamp((n_ids - first) // cnt, min=1)
    offs = torch.arange(int(indptr[-1]), device=dev) - torch.repeat_interleave(indptr[:-1], cnt)
    base = (torch.rand(cnt.numel(), device=dev, generator=g) * stride).long()
    ids = first + torch.repeat_interleave(stride, cnt) * offs + torch.repeat_interleave(base, cnt)
    assert int(ids.max()) < n_ids
    return indptr, ids.to(torch.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timing_roles():
    """R negative-role steps against none (the single-role entry), alternating, on the lists of `timing`."""
    m, epochs = 2_000, 5
    say(f"(i) one fold_in_items call, {m} new items, {epochs} epochs, sampled negatives, item bias, lr 0.05, reg_item "
        f"0.01, balance on; neg_role {NEG_ROLE} against 0 (bpr_fold_in_item_rows), alternating in one process; ms: "
        f"median  min .. max of {opt.reps}; us/step: per sequential step of the longest row, epochs * (L + R) of them")
    say(f"{'shape':34s} {'nnz':>9s} {'longest':>7s} {'R':>6s} {'T':>10s} | {'ms, R = 0':>28s} {'us/step':>7s} | "
        f"{'ms, R':>28s} {'us/step':>7s} | {'ratio':>6s} {'(L+R)/L':>7s}")
    for name, U, I, d, mean_seen, median, sigma in (("ML-20M U=138493 I=20109 d=128", 138_493, 20_109, 128, 144, 40.0, 2.0),
                                                    ("MSD U=571355 I=41140 d=256", 571_355, 41_140, 256, 59, 20.0, 1.5)):
        g = torch.Generator(device=dev).manual_seed(1)
        P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
        Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
        b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
        seen_cnt = torch.randint(1, 2 * mean_seen, (U,), device=dev, generator=g)
        seen_indptr, seen_indices = strided_csr(seen_cnt, I, 1, g)
        train_users = torch.repeat_interleave(torch.arange(U, device=dev, dtype=torch.int32), seen_cnt)
        lens = torch.clamp(torch.round(median * torch.exp(sigma * torch.randn(m, device=dev, generator=g))), 1, U // 4)
        indptr, users = strided_csr(lens.long(), U, 0, g)
        nnz, longest, T = int(indptr[-1]), int(lens.max()), train_users.numel()
        R = max(1, round(T / (I - 1))) if NEG_ROLE == "auto" else NEG_ROLE
        kw = dict(epochs=epochs, lr=0.05, reg_item=0.01, init_std=0.01, seed=3, seen_indptr=seen_indptr,
                  seen_indices=seen_indices)
        calls = {0: lambda: fold_in_items(P, Q, b, indptr, users, **kw),
                 R: lambda: fold_in_items(P, Q, b, indptr, users, neg_role=R, train_users=train_users,
                                          train_items=seen_indices, **kw)}
        ms = {0: [], R: []}
        for side in (0, R):
            calls[side]()  # warm-up
        for _ in range(opt.reps):
            for side in (0, R):
                ms[side].append(timed(calls[side]))
        med = {}
        cells = []
        for side in (0, R):
            v = sorted(ms[side])
            med[side] = v[len(v) // 2]
            cells.append(f"{med[side]:10.3f}  {v[0]:7.3f} .. {v[-1]:7.3f} {1e3 * med[side] / (epochs * (longest + side)):7.3f}")
        say(f"{name:34s} {nnz:9d} {longest:7d} {R:6d} {T:10d} | {cells[0]} | {cells[1]} | {med[R] / med[0]:6.3f} "
            f"{(longest + R) / longest:7.3f}")
        del P, Q, b, seen_indptr, seen_indices, indptr, users, train_users


def timing():
    m, epochs = 2_000, 5
    say(f"(i) one fold_in_items call, {m} new items, {epochs} epochs, sampled negatives, item bias, lr 0.05, reg_item "
        f"0.01; ms: median  min .. max of {opt.reps}")
    say(f"{'shape':34s} {'nnz':>9s} {'longest':>7s} {'balance':>7s} | {'ms':>28s} | {'M triples/s':>11s}")
    for name, U, I, d, mean_seen, median, sigma in (("ML-20M U=138493 I=20109 d=128", 138_493, 20_109, 128, 144, 40.0, 2.0),
                                                    ("MSD U=571355 I=41140 d=256", 571_355, 41_140, 256, 59, 20.0, 1.5)):
        g = torch.Generator(device=dev).manual_seed(1)
        P = (torch.rand(U, d, device=dev, generator=g) - 0.5) / d
        Q = (torch.rand(I, d, device=dev, generator=g) - 0.5) / d
        b = (torch.rand(I, device=dev, generator=g) - 0.5) / d
        seen_indptr, seen_indices = strided_csr(torch.randint(1, 2 * mean_seen, (U,), device=dev, generator=g), I, 1, g)
        lens = torch.clamp(torch.round(median * torch.exp(sigma * torch.randn(m, device=dev, generator=g))), 1, U // 4)
        indptr, users = strided_csr(lens.long(), U, 0, g)
        nnz = int(indptr[-1])
        res = {}
        for balance in (True, False):
            call = lambda: fold_in_items(P, Q, b, indptr, users, epochs=epochs, lr=0.05, reg_item=0.01, init_std=0.01,  # noqa: E731
                                         seed=3, balance=balance, seen_indptr=seen_indptr, seen_indices=seen_indices)
            res[balance] = call()
            ms = sorted(timed(call) for _ in range(opt.reps))
            med = ms[len(ms) // 2]
            say(f"{name:34s} {nnz:9d} {int(lens.max()):7d} {str(balance):>7s} | {med:10.3f}  {ms[0]:7.3f} .. {ms[-1]:7.3f} | "
                f"{epochs * nnz / med / 1e3:11.1f}")
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
        del P, Q, b, seen_indptr, seen_indices, indptr, users


def csr(rows, cols, n_rows):
    """(indptr, cols sorted by (row, col), rows sorted)"""
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
    return indptr, cols[order].astype(np.int32), rows[order].astype(np.int32)


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
    U, I = data.num_users, data.num_items
    rng = np.random.default_rng(6)
    cold = np.sort(rng.choice(np.arange(1, I), size=I0 // 10, replace=False))
    # the catalogue re-numbered: warm items keep their order in 0 .. Iw-1 (0 = the pad item), cold items follow
    new_id = np.zeros(I, np.int64)
    is_cold = np.zeros(I, bool)
    is_cold[cold] = True
    Iw = I - len(cold)
    new_id[~is_cold] = np.arange(Iw)
    new_id[cold] = Iw + np.arange(len(cold))
    tr_u, tr_i = data.users.astype(np.int64), new_id[data.items]
    ev_u = np.repeat(data.eval_users.astype(np.int64), np.diff(data.eval_indptr))
    ev_i = new_id[data.eval_items]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    # jointly: every item trains
    all_indptr, all_indices, all_users = csr(tr_u, tr_i, U)
    Pj, Qj = train(t(all_users), t(all_indices), t(all_indptr), t(all_indices), U, I, d, epochs, lr, reg, seed=7)
    # without the cold items: a catalogue of Iw items, their triples leave the training set
    warm = tr_i < Iw
    w_indptr, w_indices, w_users = csr(tr_u[warm], tr_i[warm], U)
    Pw, Qw = train(t(w_users), t(w_indices), t(w_indptr), t(w_indices), U, Iw, d, epochs, lr, reg, seed=7)
    # the cold items as a list of their own: audiences (training side) and targets (held-out side, per user)
    c_indptr, c_users, _ = csr(tr_i[~warm] - Iw, tr_u[~warm], len(cold))
    tgt = ev_i >= Iw
    e_indptr, e_items, _ = csr(ev_u[tgt], ev_i[tgt], U)
    e_users = np.flatnonzero(np.diff(e_indptr)).astype(np.int32)
    e_indptr = np.concatenate([[0], np.cumsum(np.diff(e_indptr)[e_users])]).astype(np.int64)

    # every held-out interaction, warm or cold: what an item that is only ever pushed up costs the other targets
    a_indptr, a_items, _ = csr(ev_u, ev_i, U)
    a_users = np.flatnonzero(np.diff(a_indptr)).astype(np.int32)
    a_indptr = np.concatenate([[0], np.cumsum(np.diff(a_indptr)[a_users])]).astype(np.int64)

    def ndcg(P, Q):
        cold_only = evaluate_topk(P, Q, None, t(e_users), t(e_indptr), t(e_items), t(all_indptr), t(all_indices),
                                  ks=(100,))["ndcg@100"]
        everything = evaluate_topk(P, Q, None, t(a_users), t(a_indptr), t(a_items), t(all_indptr), t(all_indices),
                                   ks=(100,))["ndcg@100"]
        return f"{cold_only:.4f}   {everything:.4f}"

    say()
    say(f"(ii) generate_latent({U0} users, {I0} items, 240,000 actions, 16 factors), d = {d}, SGD lr {lr}, reg {reg}, "
        f"{epochs} epochs of uniform-negative STREAM training; {len(cold)} items held out ({int((~warm).sum())} training "
        f"interactions to fold in from, {int(tgt.sum())} held-out interactions of {len(e_users)} users to find); "
        f"nDCG@100 in the whole catalogue of those interactions alone | of ALL {len(ev_i)} held-out interactions "
        f"({len(a_users)} users)")
    say(f"  trained jointly with everything                           {ndcg(Pj, Qj)}")
    for fe in (5, 20, 60):
        Qn = fold_in_items(Pw, Qw, None, t(c_indptr), t(c_users), epochs=fe, lr=lr, reg_item=reg, init_std=0.1, seed=8,
                           seen_indptr=t(w_indptr), seen_indices=t(w_indices))
        say(f"  folded in against the tables trained without them, {fe:2d} epochs   {ndcg(Pw, torch.cat((Qw, Qn)))}")
        if NEG_ROLE != 0:
            Qn, roles = fold_in_items(Pw, Qw, None, t(c_indptr), t(c_users), epochs=fe, lr=lr, reg_item=reg, init_std=0.1,
                                      seed=8, seen_indptr=t(w_indptr), seen_indices=t(w_indices), neg_role=NEG_ROLE,
                                      train_users=t(w_users), train_items=t(w_indices), return_roles=True)
            per = roles.numel() // (fe * len(cold))
            say(f"  the same with neg_role {NEG_ROLE} (R = {per}, {int((roles < 0).sum())} steps skipped), {fe:2d} epochs"
                f"   {ndcg(Pw, torch.cat((Qw, Qn)))}")
    g = torch.Generator(device=dev).manual_seed(8)
    Qn = torch.randn(len(cold), d, device=dev, generator=g) * 0.1
    say(f"  untrained rows (N(0, 0.1^2)) beside those tables           {ndcg(Pw, torch.cat((Qw, Qn)))}")


say(f"device {torch.cuda.get_device_name(0)}")
if not opt.skip_timing:
    timing_roles() if NEG_ROLE != 0 else timing()
if not opt.skip_study:
    study()
Path(opt.out).parent.mkdir(parents=True, exist_ok=True)
with open(opt.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
