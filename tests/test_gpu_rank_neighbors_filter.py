"""The item filter of `rank_items` / `evaluate_ranked` (`bpr_rank_rows_filtered`) and of `neighbors` / `similar_items` /
`similar_users` (`bpr_neighbors_rows_filtered`) on the GPU.  Ranks and ids are compared as integers, scores bit by bit.

The oracle is the COMPACTED problem run through the parent kernel (no filter: the `FILT = false` instantiation, which
is not the code under test).  For a filter F: keep = [0] + the eligible ids ascending; Q' = Q[keep], the bias
likewise; the seen and target CSRs restricted to keep and renumbered.  The renumbering is monotone, so ties by
ascending id survive; a row's dot product does not depend on the table around it, so scores are the same bits.

Shapes: I in {129, 300, 1000} (two tiles; three with a partial last one; eight), d in {8, 21, 128}, every shape with
16-byte aligned tables and with tables offset by one float (the element-load instantiations), n in {1, 65} (65 rows
span two row tiles), item_slices in {1, 3}.  Filters: all ones; half at random; one whole empty tile in the middle;
only the last partial tile non-empty; all zero; bit 0 and bits at or past I set on purpose."""
import functools

import numpy as np
import pytest
import torch

import filter_model as fm

pytestmark = pytest.mark.gpu

F32 = np.float32
U, N_ROWS = 40, 65
SHAPES = [(I, d, off) for I in (129, 300, 1000) for d in (8, 21, 128) for off in (0, 1)]
SHAPE_IDS = [f"I{I}-d{d}-{'offset' if off else 'aligned'}" for I, d, off in SHAPES]


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def table(x, off):
    """a float32 table on the device, its start 16-byte aligned (off = 0) or one float past that (off = 1)"""
    x = np.ascontiguousarray(x, dtype=F32)
    flat = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    out = flat[off:off + x.size].view(x.shape)
    out.copy_(torch.from_numpy(x))
    assert out.data_ptr() % 16 == 4 * off
    return out


def filters(I):
    """name -> uint32 words, as the kernels get them"""
    tiles = -(-I // 128)
    idx = np.arange(I)
    rng = np.random.default_rng(I)
    half = rng.random(I) < 0.5
    out = {"all-ones": fm.pack(np.ones(I, bool)), "half": fm.pack(half), "all-zero": fm.pack(np.zeros(I, bool)),
           "empty-middle-tile": fm.pack(idx // 128 != tiles // 2),
           "last-tile-only": fm.pack(idx // 128 == tiles - 1)}
    dirty = fm.pack(half | (idx == 0))
    tail = np.zeros(32 * len(dirty), bool)
    tail[I:] = True
    out["bit-0-and-tail-bits"] = dirty | np.packbits(tail, bitorder="little").view(np.uint32)
    return out


def csr(rows):
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32))


def restrict(rows, remap):
    """rows of ids -> (rows of the kept ids renumbered, for each row the positions that were kept)"""
    kept, where = [], []
    for r in rows:
        r = np.asarray(r, np.int64)
        ok = (r >= 0) & (r < len(remap))
        ok[ok] = remap[r[ok]] >= 0
        kept.append(remap[r[ok]].astype(np.int32))
        where.append(np.flatnonzero(ok))
    return kept, where


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(I, d, off):
    rng = np.random.default_rng(1000 * I + 10 * d + off)
    c = Case()
    c.I, c.d, c.off = I, d, off
    c.P = (0.3 * rng.standard_normal((U, d))).astype(F32)
    c.Q = (0.3 * rng.standard_normal((I, d))).astype(F32)
    c.b = (0.3 * rng.standard_normal(I)).astype(F32)
    for _ in range(I // 4):  # twins: equal scores, ordered by id
        a, b = rng.integers(1, I, 2)
        c.Q[a], c.b[a] = c.Q[b], c.b[b]
    c.seen = [np.zeros(0, np.int32) if u == 0 else np.arange(1, I, dtype=np.int32) if u == 1 else
              (np.flatnonzero(rng.random(I - 1) < 0.2) + 1).astype(np.int32) for u in range(U)]
    c.users = np.concatenate([np.arange(U), rng.integers(0, U, N_ROWS - U)]).astype(np.int32)
    rng.shuffle(c.users)
    c.tgts = []
    for r, u in enumerate(c.users):  # unseen, seen and item 0 among them; row 7 is as long as a row may be
        m = 112 if r == 7 else int(rng.integers(0, 9))
        t = rng.choice(np.arange(1, I), min(m, I - 1), replace=False).astype(np.int32)
        if r % 5 == 0:
            t = np.concatenate([t[:max(len(t) - 1, 0)], [0]]).astype(np.int32)
        c.tgts.append(t)
    c.t = (table(c.P, off), table(c.Q, off), dev(c.b))
    c.seen_dev = tuple(dev(x) for x in csr(c.seen))
    c.words = filters(I)
    c.f = {k: dev(w.view(np.int32)) for k, w in c.words.items()}
    return c


def rank_call(c, rows, name, **kw):
    from revisit_bpr.ranks import rank_items

    tptr, titems = csr([c.tgts[r] for r in rows])
    out = rank_items(*c.t, dev(c.users[rows]), dev(tptr), dev(titems), *c.seen_dev,
                     item_filter=None if name is None else c.f[name], **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@functools.lru_cache(maxsize=None)
def compacted(I, d, off, name):
    """the parent kernel on the compacted problem, scattered back to the places of the original targets; the dropped
    ones hold -1 / -1 / -inf"""
    from revisit_bpr.ranks import rank_items

    c = case(I, d, off)
    ok = fm.eligible_items(c.words[name], I)
    keep = np.concatenate([[0], np.flatnonzero(ok)])
    remap = np.full(I, -1, np.int64)
    remap[keep] = np.arange(len(keep))
    seen2, _ = restrict(c.seen, remap)
    tg2, where = restrict(c.tgts, remap)
    tptr, titems = csr(tg2)
    out = rank_items(table(c.P, off), table(c.Q[keep], off), dev(c.b[keep]), dev(c.users), dev(tptr), dev(titems),
                     *(dev(x) for x in csr(seen2)))   # NO filter
    torch.cuda.synchronize()
    rank, nb, sc = (o.cpu().numpy() for o in out)
    full = []
    for r in range(N_ROWS):
        m = len(c.tgts[r])
        row = [np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.full(m, -np.inf, F32)]
        for dst, src in zip(row, (rank, nb, sc)):
            dst[where[r]] = src[tptr[r]:tptr[r + 1]]
        full.append(row)
    return full, keep


def want_rows(full, rows):
    return [np.concatenate([full[r][j] for r in rows] + [np.zeros(0, full[0][j].dtype)]) for j in range(3)]


def same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


ALL = np.arange(N_ROWS)


# ---- (a) rank_items(item_filter=F) is the parent on the compacted problem --------------------------------------------
@pytest.mark.parametrize("I, d, off", SHAPES, ids=SHAPE_IDS)
def test_filtered_ranks_are_the_parents_on_the_compacted_problem(I, d, off):
    c = case(I, d, off)
    for name in c.words:
        full, keep = compacted(I, d, off, name)
        ok = np.zeros(I, bool)
        ok[keep[1:]] = True
        for s in (1, 3):
            for rows in (ALL, np.array([7])):
                got = rank_call(c, rows, name, item_slices=s)
                assert same(got, want_rows(full, rows)), (name, s, len(rows))
                t = np.concatenate([c.tgts[r] for r in rows])
                out = ~ok[t]                                   # a target whose bit is clear (item 0 among them)
                assert (got[0][out] == -1).all() and (got[1][out] == -1).all() and (got[2][out] == -np.inf).all()
    for s in (1, 3):
        assert same(rank_call(c, ALL, "all-ones", item_slices=s), rank_call(c, ALL, None, item_slices=s)), s
    got = rank_call(c, ALL, "all-zero")
    assert (got[0] == -1).all() and (got[1] == -1).all() and (got[2] == -np.inf).all()


# ---- (b) the seen cursors across a run of skipped tiles --------------------------------------------------------------
@pytest.mark.parametrize("d, off", [(8, 0), (21, 0), (128, 1)], ids=["d8", "d21", "d128-offset"])
def test_seen_cursors_across_skipped_tiles(d, off):
    """I = 1000: tiles 2, 3 and 4 hold no eligible item, tile 5 is walked behind them.  Every user has seen items
    inside the skipped run, and all but user 3, whose list ENDS inside the run, inside tile 5 as well; user 4's list
    has 4 k + 1 entries, so the four cursors are uneven; row 0 holds 112 targets."""
    from revisit_bpr.ranks import rank_items

    I = 1000
    rng = np.random.default_rng(77 + d)
    P = (0.3 * rng.standard_normal((U, d))).astype(F32)
    Q = (0.3 * rng.standard_normal((I, d))).astype(F32)
    idx = np.arange(I)
    mask = ~((idx >= 256) & (idx < 640)) & (rng.random(I) < 0.8)
    mask[640:768] |= rng.random(128) < 0.5
    words = fm.pack(mask)
    seen = []
    for u in range(U):
        inside = rng.choice(np.arange(256, 640), int(rng.integers(3, 60)), replace=False)
        after = rng.choice(np.arange(640, 768), int(rng.integers(5, 40)), replace=False)
        rest = rng.choice(np.concatenate([np.arange(1, 256), np.arange(768, I)]), int(rng.integers(0, 80)), replace=False)
        s = np.unique(np.concatenate([inside, after, rest]))
        if u == 3:
            s = s[s < 500]                     # ends inside the skipped run
        if u == 4:
            s = s[:4 * ((len(s) - 1) // 4) + 1]
            assert len(s) % 4 == 1 and s.max() >= 640
        seen.append(s.astype(np.int32))
    assert all(((s >= 256) & (s < 640)).any() for s in seen)
    assert all(((s >= 640) & (s < 768)).any() for u, s in enumerate(seen) if u != 3) and seen[3].max() < 640
    users = np.arange(U, dtype=np.int32)
    tgts = [rng.choice(np.arange(1, I), 112 if u == 0 else int(rng.integers(1, 9)), replace=False).astype(np.int32)
            for u in range(U)]
    ok = fm.eligible_items(words, I)
    keep = np.concatenate([[0], np.flatnonzero(ok)])
    remap = np.full(I, -1, np.int64)
    remap[keep] = np.arange(len(keep))
    seen2, _ = restrict(seen, remap)
    tg2, where = restrict(tgts, remap)
    tptr2, ti2 = csr(tg2)
    ref = rank_items(table(P, off), table(Q[keep], off), None, dev(users), dev(tptr2), dev(ti2),
                     *(dev(x) for x in csr(seen2)))
    ref = [o.cpu().numpy() for o in ref]
    tptr, ti = csr(tgts)
    want = [np.full(len(ti), -1, np.int32), np.full(len(ti), -1, np.int32), np.full(len(ti), -np.inf, F32)]
    for u in range(U):
        for dst, src in zip(want, ref):
            dst[tptr[u] + where[u]] = src[tptr2[u]:tptr2[u + 1]]
    Pd, Qd, f = table(P, off), table(Q, off), dev(words.view(np.int32))
    for s in (1, 2, 3, 8):
        got = rank_items(Pd, Qd, None, dev(users), dev(tptr), dev(ti), *(dev(x) for x in csr(seen)), item_filter=f,
                         item_slices=s)
        assert same([o.cpu().numpy() for o in got], want), s


# ---- (c) independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I, d, off", [(1000, 21, 0), (300, 128, 0), (1000, 8, 1)],
                         ids=["I1000-d21", "I300-d128", "I1000-d8-offset"])
def test_result_does_not_depend_on_n_row_order_or_slices(I, d, off):
    c = case(I, d, off)
    perm = np.random.default_rng(3).permutation(N_ROWS)
    for name in ("half", "empty-middle-tile", "last-tile-only"):
        base = rank_call(c, ALL, name, item_slices=1)
        tptr, _ = csr(c.tgts)
        for s in (0, 2, 3, 8):
            assert same(rank_call(c, ALL, name, item_slices=s), base), (name, s)
        for s in (1, 3):
            got = rank_call(c, perm, name, item_slices=s)
            want = [np.concatenate([x[tptr[r]:tptr[r + 1]] for r in perm]) for x in base]
            assert same(got, want), (name, s)
            for r in (0, 7, 64):
                one = rank_call(c, np.array([r]), name, item_slices=s)
                assert same(one, [x[tptr[r]:tptr[r + 1]] for x in base]), (name, s, r)


# ---- (d) evaluate_ranked ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["masked-negatives", "eligible-negatives"])
@pytest.mark.parametrize("I, d, off", [(300, 21, 0), (1000, 128, 0), (129, 8, 1)],
                         ids=["I300-d21", "I1000-d128", "I129-d8-offset"])
def test_evaluate_ranked_is_evaluate_ranked_on_the_compacted_problem(I, d, off, masked):
    from revisit_bpr.evaluation import evaluate_ranked

    c = case(I, d, off)
    ks = (1, 5, 20, 100)
    users = np.arange(U, dtype=np.int32)
    rng = np.random.default_rng(I + d)
    tgts = [rng.choice(np.arange(0, I), int(rng.integers(0, 12)), replace=False).astype(np.int32) for _ in range(U)]
    eptr, eitems = csr(tgts)
    for name in c.words:
        ok = fm.eligible_items(c.words[name], I)
        keep = np.concatenate([[0], np.flatnonzero(ok)])
        I2 = len(keep)
        remap = np.full(I, -1, np.int64)
        remap[keep] = np.arange(I2)
        seen2, _ = restrict(c.seen, remap)
        tg2, _ = restrict(tgts, remap)
        got, per = evaluate_ranked(*c.t, dev(users), dev(eptr), dev(eitems), *c.seen_dev, ks=ks, auc=True,
                                   extra=True, per_user=True, masked_negatives=masked, item_filter=c.f[name])
        want, wper = evaluate_ranked(table(c.P, off), table(c.Q[keep], off), dev(c.b[keep]), dev(users),
                                     *(dev(x) for x in csr(tg2)), *(dev(x) for x in csr(seen2)), ks=ks, auc=True,
                                     extra=True, per_user=True, masked_negatives=masked)
        assert set(got) == set(want) and set(per) == set(wper)
        wper = {k: v.cpu().numpy() for k, v in wper.items()}
        if masked:
            # the compacted side lacks the I - I2 filtered-out items, which are negatives below every positive:
            # its n_neg, and each retrievable positive's count of negatives below it, are short by that constant
            T = np.array([len(t) for t in tg2], np.float64)                          # (ids are unique in a row)
            m = np.array([int(((t > 0) & ~np.isin(t, s)).sum()) for t, s in zip(tg2, seen2)], np.float64)
            pairs = np.rint(np.nan_to_num(wper["auc"]) * T * (I2 - T))
            with np.errstate(invalid="ignore", divide="ignore"):
                wper["auc"] = (pairs + m * (I - I2)) / (T * (I - T))
        for key in per:
            g = per[key].cpu().numpy()
            assert g.dtype == np.float64
            if "@" in key and int(key.split("@")[1]) > I2:
                continue  # k > I behaves as k = I, and the two sides differ in I: compared at the cutoffs up to I2
            assert np.array_equal(g, wper[key], equal_nan=True), (name, key)
            mean = wper[key].sum() / U
            assert (np.isnan(got[key]) and np.isnan(mean)) or abs(got[key] - mean) <= 1e-12 * abs(mean), (name, key)


# ---- (e) neighbors ---------------------------------------------------------------------------------------------------
def nbr_call(X, T, rows, k, f, **kw):
    from revisit_bpr.similar import neighbors

    ids, sc = neighbors(X, T, dev(rows), k, item_filter=f, **kw)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


@pytest.mark.parametrize("N, d, off", SHAPES, ids=[s.replace("I", "N", 1) for s in SHAPE_IDS])
def test_filtered_neighbors_are_the_parents_on_the_kept_rows(N, d, off):
    rng = np.random.default_rng(7 * N + d + off)
    Tn = (0.3 * rng.standard_normal((N, d))).astype(F32)
    for _ in range(N // 4):  # twins and a zero row
        a, b = rng.integers(0, N, 2)
        Tn[a] = Tn[b]
    Tn[min(5, N - 1)] = 0
    T = table(Tn, off)
    rows_all = np.concatenate([[0, 1, N - 1], rng.integers(0, N, N_ROWS - 3)]).astype(np.int32)
    idx = np.arange(N)
    fs = dict(filters(N))
    fs["three-rows"] = fm.pack(np.isin(idx, [0, 2, N - 1]))      # fewer than k
    fs["keeps-row-0"] = fm.pack((idx % 3 == 0))
    for name, words in fs.items():
        f = dev(words.view(np.int32))
        stored = np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool)
        for first in (0, 1):
            keep = np.flatnonzero(stored & (idx >= first))
            remap = np.full(N, -1, np.int64)
            remap[keep] = np.arange(len(keep))
            Tk = table(Tn[keep], off) if len(keep) else None
            for metric in ("dot", "cosine"):
                for k in (5, 128):
                    for excl in (None, rows_all):             # the query itself: in F for some rows, not for others
                        ex2 = None if excl is None else remap[excl].astype(np.int32)
                        if len(keep):
                            wi, ws = nbr_call(T, Tk, rows_all, k, None, metric=metric, first=0,
                                              exclude=None if ex2 is None else dev(ex2))
                            wi = np.where(wi >= 0, keep[np.maximum(wi, 0)], -1).astype(np.int32)
                        else:
                            wi, ws = np.full((N_ROWS, k), -1, np.int32), np.full((N_ROWS, k), -np.inf, F32)
                        for s in (1, 3):
                            for rows in (ALL, np.array([0])):
                                gi, gs = nbr_call(T, T, rows_all[rows], k, f, metric=metric, first=first,
                                                  exclude=None if excl is None else dev(excl[rows]), item_slices=s)
                                what = (name, first, metric, k, excl is None, s, len(rows))
                                assert np.array_equal(gi, wi[rows]), what
                                assert np.array_equal(bits(gs), bits(ws[rows])), what
                                live = gi[gi >= 0]
                                assert stored[live].all() and (live >= first).all(), what
        if name == "three-rows":
            gi, gs = nbr_call(T, T, rows_all, 5, f, metric="dot", first=1)
            assert ((gi >= 0).sum(axis=1) <= 2).all() and (gi[:, 2:] == -1).all() and (gs[:, 2:] == -np.inf).all()
        if name == "all-ones":
            for first in (0, 1):
                for metric in ("dot", "cosine"):
                    a = nbr_call(T, T, rows_all, 20, f, metric=metric, first=first, exclude=dev(rows_all))
                    b = nbr_call(T, T, rows_all, 20, None, metric=metric, first=first, exclude=dev(rows_all))
                    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- (f) the Python surface and the refusals -------------------------------------------------------------------------
def test_engine_methods_give_what_the_module_functions_give():
    from revisit_bpr.engine import Engine
    from revisit_bpr.item_filter import pack_item_filter
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.similar import similar_items, similar_users

    c = case(300, 128, 0)
    f = c.f["half"]
    fu = pack_item_filter(U, deny=[3, 4], device="cuda")
    tptr, titems = (dev(x) for x in csr(c.tgts))
    users = dev(c.users)
    e = Engine(c.t[0].clone(), c.t[1].clone(), c.t[2].clone())
    e.bind_seen_csr(*c.seen_dev)
    ids = torch.arange(1, 40, dtype=torch.int32, device="cuda")
    pairs = [(e.rank_items(users, tptr, titems, item_filter=f, item_slices=2),
              rank_items(*c.t, users, tptr, titems, *c.seen_dev, item_filter=f)),
             (e.rank_items(users, tptr, titems, exclude_seen=False, item_filter=f),
              rank_items(*c.t, users, tptr, titems, item_filter=f)),
             (e.similar_items(ids, 10, item_filter=f), similar_items(c.t[1], ids, 10, item_filter=f)),
             (e.similar_users(ids, 10, "dot", item_filter=fu), similar_users(c.t[0], ids, 10, "dot", item_filter=fu))]
    for got, want in pairs:
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    got = e.similar_users(torch.tensor([7], dtype=torch.int32, device="cuda"), U, "dot", item_filter=fu)[0]
    live = got[got >= 0].tolist()
    assert sorted(live) == [u for u in range(U) if u not in (3, 4, 7)] and 0 in live    # user 0 is a user
    e.close()


def test_model_methods_give_what_the_module_functions_give():
    from revisit_bpr.datasets import synthetic
    from revisit_bpr.item_filter import pack_item_filter
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.similar import similar_items, similar_users

    data = synthetic.generate(500, 300, 9000, median_per_user=15, seed=1)
    torch.manual_seed(3)
    model = BPR(fuse_forward=True, reg_alphas={"all": 0.001},
                logits_model=MF(torch.nn.Embedding(data.num_users, 32, padding_idx=0),
                                torch.nn.Embedding(data.num_items, 32, padding_idx=0),
                                item_bias=True, user_bias=False)).cuda()
    seen = (dev(data.indptr), dev(data.indices))
    model.bind_seen_csr(*seen)
    users = torch.arange(0, 100, dtype=torch.int32, device="cuda")
    tptr = torch.arange(0, 301, 3, dtype=torch.int64, device="cuda")
    titems = torch.randint(1, data.num_items, (300,), dtype=torch.int32, device="cuda")
    f = pack_item_filter(data.num_items, deny=torch.arange(0, data.num_items, 3), device="cuda")
    fu = pack_item_filter(data.num_users, deny=torch.arange(1, data.num_users, 2), device="cuda")
    sd = model.state_dict()
    t = (sd["logits_model._user_emb.weight"], sd["logits_model._item_emb.weight"], sd["logits_model._item_bias"])
    pairs = [(model.rank_items(users, tptr, titems, item_filter=f),
              rank_items(*t, users, tptr, titems, *seen, item_filter=f)),
             (model.similar_items(users + 1, 10, item_filter=f), similar_items(t[1], users + 1, 10, item_filter=f)),
             (model.similar_users(users, 10, item_filter=fu), similar_users(t[0], users, 10, item_filter=fu))]
    for got, want in pairs:
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    out = (titems.long() % 3 == 0)
    assert (pairs[0][0][0][out] == -1).all()
    items, others = pairs[1][0][0], pairs[2][0][0]      # (user 0's row is zero: under cosine its row is padding)
    assert (items[items >= 0].long() % 3 != 0).all() and (others[others >= 0].long() % 2 == 0).all()
    assert (items >= 0).any() and (others >= 0).any()


def test_a_filter_on_another_device_is_refused_before_the_launch():
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.similar import neighbors

    c = case(300, 128, 0)
    tptr, titems = (dev(x) for x in csr(c.tgts))
    on_cpu = c.f["half"].cpu()
    with pytest.raises(RuntimeError, match="on a ROCm device"):
        rank_items(*c.t, dev(c.users), tptr, titems, *c.seen_dev, item_filter=on_cpu)
    with pytest.raises(RuntimeError, match="on a ROCm device"):
        neighbors(c.t[1], c.t[1], dev(c.users), 5, item_filter=on_cpu)


def test_misaligned_filter_is_refused_under_the_new_functions_names():
    from revisit_bpr import native
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.similar import neighbors

    c = case(300, 128, 0)
    tptr, titems = (dev(x) for x in csr(c.tgts))
    room = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert room.data_ptr() % 16 == 0
    with pytest.raises(native.BprError, match="bpr_rank_rows_filtered: item_filter must be 16-byte aligned"):
        rank_items(*c.t, dev(c.users), tptr, titems, *c.seen_dev, item_filter=room[1:13])
    with pytest.raises(native.BprError, match="bpr_neighbors_rows_filtered: item_filter must be 16-byte aligned"):
        neighbors(c.t[1], c.t[1], dev(c.users), 5, item_filter=room[1:13])
