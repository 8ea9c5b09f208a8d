"""What the serving entry points refuse, and in which words, on a machine without a GPU: every `_workspace`,
`_slices`, `_layout`, `_rows` and `bpr_test_*_plan` entry of the seven serving families (topk, retrieve, sample,
neighbors, rank, rerank, diversify) with one malformed argument at a time, the return code and the WHOLE
`bpr_last_error()` string; for two faults at once, which one is reported; and the refusals of the Python wrappers
that CPU tensors reach, type and full message.  The messages are written out here: they are part of the interface,
and the host prologue the entry points share (csrc/bpr_serving_host.h, revisit_bpr/_serving.py) must not move one.

Nothing here touches a device: every `_rows` call is one that returns before its first runtime call."""
import ctypes
from ctypes import POINTER, byref, c_int, c_int32, c_int64

import pytest
import torch

INVALID = -1
B31 = 2 ** 31
PLAN_HOOKS = ("bpr_test_topk_plan", "bpr_test_retrieve_plan", "bpr_test_neighbors_plan", "bpr_test_rank_plan",
              "bpr_test_rerank_plan", "bpr_test_diversify_plan")


def lib():
    from revisit_bpr import native

    L = native.load()
    for name in PLAN_HOOKS:
        fn = getattr(L, name)
        fn.restype = c_int
        fn.argtypes = [POINTER(c_int64)] * (2 if name in ("bpr_test_rerank_plan", "bpr_test_diversify_plan") else 3)
    return L


def last():
    return lib().bpr_last_error().decode()


def o64(a):
    return None if a.get("null_out") else byref(c_int64())


def o32(a):
    return None if a.get("null_out") else byref(c_int32())


def hook(name, *vals):
    out, bounds = (c_int64 * 16)(), (c_int64 * 80)()
    args = [(c_int64 * len(vals))(*vals), out]
    if name not in ("bpr_test_rerank_plan", "bpr_test_diversify_plan"):
        args.append(bounds)
    return getattr(lib(), name)(*args)


# ---- the sliced top-k families: an entry is (name, call(a), needs k).  `a` holds n, rows, d, k, item_slices and what
# the `_rows` entries want besides; 1 stands for a pointer that is never followed.
TOPK_GOOD = dict(n=4, rows=100, d=8, k=10, item_slices=0, metric=0, first=0, temperature=1.0, P=1, Q=1, users=1,
                 items=1, scores=1, ws=None, ws_bytes=0)


def topk_rows(a):
    return lib().bpr_topk_rows(a["P"], a["Q"], None, a["rows"], a["d"], a["users"], a["n"], None, None, a["k"],
                               a["item_slices"], a["ws"], a["ws_bytes"], a["items"], a["scores"], None)


def retrieve_rows(a):
    return lib().bpr_retrieve_rows(a["P"], a["Q"], None, a["rows"], a["d"], a["users"], a["n"], None, None, a["k"],
                                   a["item_slices"], a["ws"], a["ws_bytes"], a["items"], a["scores"], None)


def sample_rows(a):
    return lib().bpr_sample_rows(a["P"], a["Q"], None, a["rows"], a["d"], a["users"], a["n"], None, None, None, a["k"],
                                 a["temperature"], 0, a["item_slices"], a["ws"], a["ws_bytes"], a["items"],
                                 a["scores"], None, a.get("log_z"), None)


def neighbors_rows(a):
    return lib().bpr_neighbors_rows(a["P"], a["Q"], a["rows"], a["d"], a["users"], a["n"], None, a["first"],
                                    a["metric"], a["k"], a["item_slices"], a["ws"], a["ws_bytes"], a["items"],
                                    a["scores"], None)


def rank_rows(a):
    return lib().bpr_rank_rows(a["P"], a["Q"], None, a["rows"], a["d"], a["users"], a["n"], a.get("tptr", 1), 1, None,
                               None, a["item_slices"], a["ws"], a["ws_bytes"], 1, 1, 1, None)


def shp(a):
    return a["n"], a["rows"], a["d"], a["k"], a["item_slices"]


TOPK_ENTRIES = {  # name -> (call, largest k, the rows' name)
    "bpr_topk_workspace": (lambda a: lib().bpr_topk_workspace(*shp(a), o64(a)), 128, "I"),
    "bpr_topk_slices": (lambda a: lib().bpr_topk_slices(*shp(a), o32(a)), 128, "I"),
    "bpr_topk_rows": (topk_rows, 128, "I"),
    "bpr_test_topk_plan": (lambda a: hook("bpr_test_topk_plan", *shp(a), 256), 128, "I"),
    "bpr_retrieve_workspace": (lambda a: lib().bpr_retrieve_workspace(*shp(a), o64(a)), 1024, "I"),
    "bpr_retrieve_slices": (lambda a: lib().bpr_retrieve_slices(*shp(a), o32(a)), 1024, "I"),
    "bpr_retrieve_rows": (retrieve_rows, 1024, "I"),
    "bpr_test_retrieve_plan": (lambda a: hook("bpr_test_retrieve_plan", *shp(a), 256), 1024, "I"),
    "bpr_sample_workspace": (lambda a: lib().bpr_sample_workspace(*shp(a), 1, o64(a)), 128, "I"),
    "bpr_sample_slices": (lambda a: lib().bpr_sample_slices(*shp(a), o32(a)), 128, "I"),
    "bpr_sample_rows": (sample_rows, 128, "I"),
    "bpr_neighbors_workspace": (lambda a: lib().bpr_neighbors_workspace(a["n"], a["rows"], a["d"], a["k"], a["metric"],
                                                                        a["item_slices"], o64(a)), 128, "N"),
    "bpr_neighbors_slices": (lambda a: lib().bpr_neighbors_slices(*shp(a), o32(a)), 128, "N"),
    "bpr_neighbors_rows": (neighbors_rows, 128, "N"),
    "bpr_test_neighbors_plan": (lambda a: hook("bpr_test_neighbors_plan", a["n"], a["rows"], a["d"], a["k"],
                                               a["metric"], a["item_slices"], 256), 128, "N"),
}
RANK_ENTRIES = {
    "bpr_rank_workspace": lambda a: lib().bpr_rank_workspace(a["n"], a["rows"], a["d"], a["item_slices"], o64(a)),
    "bpr_rank_slices": lambda a: lib().bpr_rank_slices(a["n"], a["rows"], a["d"], a["item_slices"], o32(a)),
    "bpr_rank_rows": rank_rows,
    "bpr_test_rank_plan": lambda a: hook("bpr_test_rank_plan", a["n"], a["rows"], a["d"], a["item_slices"], 256),
}


def refused(call, a, message):
    assert call(a) == INVALID
    assert last() == message


@pytest.mark.parametrize("who", sorted(TOPK_ENTRIES))
def test_topk_families_refuse_each_malformed_shape(who):
    call, kmax, R = TOPK_ENTRIES[who]
    good = dict(TOPK_GOOD)
    if not who.endswith("_rows"):
        assert call(good) == 0  # (a `_rows` call of a good shape would launch)
    rows_msg = f"{who}: n must be >= 0 and {R} in [1, 2^31)"
    d_msg = f"{who}: d must be in [1, 1024]"
    k_msg = f"{who}: k must be in [1, {kmax}]"
    s_msg = f"{who}: item_slices must be 0 (choose) or in [1, 64]"
    for kw, message in [
        (dict(n=-1), rows_msg), (dict(rows=0), rows_msg), (dict(rows=B31), rows_msg),
        (dict(d=0), d_msg), (dict(d=1025), d_msg),
        (dict(k=0), k_msg), (dict(k=kmax + 1), k_msg),
        (dict(item_slices=-1), s_msg), (dict(item_slices=65), s_msg),
        (dict(n=B31), f"{who}: n must be below 2^31"),
        # two faults at once: the clauses' order is n / rows, d, k, item_slices, n's upper bound
        (dict(n=-1, d=0), rows_msg), (dict(rows=0, k=0), rows_msg), (dict(d=0, k=0), d_msg),
        (dict(d=1025, item_slices=-1), d_msg), (dict(k=0, item_slices=65), k_msg), (dict(k=kmax + 1, n=B31), k_msg),
        (dict(item_slices=65, n=B31), s_msg),
    ]:
        refused(call, {**good, **kw}, message)


@pytest.mark.parametrize("who", sorted(RANK_ENTRIES))
def test_rank_family_refuses_each_malformed_shape(who):
    call = RANK_ENTRIES[who]
    good = dict(TOPK_GOOD)
    if not who.endswith("_rows"):
        assert call(good) == 0
    rows_msg = f"{who}: n must be >= 0 and I in [1, 2^31)"
    d_msg = f"{who}: d must be in [1, 1024]"
    s_msg = f"{who}: item_slices must be 0 (choose) or in [1, 64]"
    n_msg = f"{who}: n must be below 2^31 / 112"
    for kw, message in [
        (dict(n=-1), rows_msg), (dict(rows=0), rows_msg), (dict(rows=B31), rows_msg),
        (dict(d=0), d_msg), (dict(d=1025), d_msg),
        (dict(item_slices=-1), s_msg), (dict(item_slices=65), s_msg),
        (dict(n=(B31 - 1) // 112 + 1), n_msg), (dict(n=B31), n_msg),
        (dict(n=-1, d=0), rows_msg), (dict(d=0, item_slices=65), d_msg), (dict(item_slices=65, n=B31), s_msg),
    ]:
        refused(call, {**good, **kw}, message)
    if not who.endswith("_rows"):
        assert call({**good, "n": (B31 - 1) // 112}) == 0  # rank's own bound, from below


@pytest.mark.parametrize("who, name", [
    ("bpr_topk_workspace", "bytes_host"), ("bpr_topk_slices", "slices_host"),
    ("bpr_retrieve_workspace", "bytes_host"), ("bpr_retrieve_slices", "slices_host"),
    ("bpr_sample_workspace", "bytes_host"), ("bpr_sample_slices", "slices_host"),
    ("bpr_neighbors_workspace", "bytes_host"), ("bpr_neighbors_slices", "slices_host"),
    ("bpr_rank_workspace", "bytes_host"), ("bpr_rank_slices", "slices_host"),
])
def test_a_null_out_pointer_is_refused_before_the_shape(who, name):
    call = TOPK_ENTRIES[who][0] if who in TOPK_ENTRIES else RANK_ENTRIES[who]
    refused(call, {**TOPK_GOOD, "null_out": True}, f"{who}: {name} is NULL")
    refused(call, {**TOPK_GOOD, "null_out": True, "n": -1, "d": 0}, f"{who}: {name} is NULL")


def test_neighbors_metric_and_first():
    metric_msg = ": metric must be BPR_SIM_DOT (0) or BPR_SIM_COSINE (1)"
    for who in ("bpr_neighbors_workspace", "bpr_neighbors_rows", "bpr_test_neighbors_plan"):
        call = TOPK_ENTRIES[who][0]
        for metric in (-1, 2):
            refused(call, {**TOPK_GOOD, "metric": metric}, who + metric_msg)
        refused(call, {**TOPK_GOOD, "metric": 2, "k": 0}, f"{who}: k must be in [1, 128]")  # the shape comes first
        refused(call, {**TOPK_GOOD, "metric": 2, "n": B31}, f"{who}: n must be below 2^31")
    assert TOPK_ENTRIES["bpr_neighbors_slices"][0]({**TOPK_GOOD, "metric": 2}) == 0  # (takes no metric)
    refused(neighbors_rows, {**TOPK_GOOD, "first": -1}, "bpr_neighbors_rows: first must be >= 0")
    refused(neighbors_rows, {**TOPK_GOOD, "first": -1, "metric": 2}, "bpr_neighbors_rows" + metric_msg)
    refused(neighbors_rows, {**TOPK_GOOD, "first": -1, "P": None}, "bpr_neighbors_rows: first must be >= 0")


def test_sample_temperature():
    message = "bpr_sample_rows: temperature must be finite and > 0, and so must 1 / temperature"
    for t in (0.0, -1.0, float("inf"), float("nan"), 1e-46, 1e-39):  # (1 / 1e-39 is inf in float32)
        refused(sample_rows, {**TOPK_GOOD, "temperature": t}, message)
    refused(sample_rows, {**TOPK_GOOD, "temperature": 0.0, "k": 0}, "bpr_sample_rows: k must be in [1, 128]")
    refused(sample_rows, {**TOPK_GOOD, "temperature": 0.0, "P": None}, message)  # before the tables


NULL_TABLES = {
    "bpr_topk_rows": "bpr_topk_rows: P, Q, users, items_out or scores_out is NULL",
    "bpr_retrieve_rows": "bpr_retrieve_rows: P, Q, users, items_out or scores_out is NULL",
    "bpr_sample_rows": "bpr_sample_rows: P, Q, users, items_out or scores_out is NULL",
    "bpr_neighbors_rows": "bpr_neighbors_rows: X, T, rows, ids_out or scores_out is NULL",
}


@pytest.mark.parametrize("who", sorted(NULL_TABLES))
def test_rows_null_tables_and_workspace(who):
    call = TOPK_ENTRIES[who][0]
    one = {**TOPK_GOOD, "n": 1}
    for name in ("P", "Q", "users", "items", "scores"):
        refused(call, {**one, name: None}, NULL_TABLES[who])
        assert call({**one, name: None, "n": 0}) == 0  # no rows: the tables are not looked at
    refused(call, {**one, "P": None, "d": 0}, f"{who}: d must be in [1, 1024]")  # the shape comes first
    # 4 slices of 5,000 rows: the partial lists are 1 x 4 x 10 x 8 bytes, and every family needs at least those
    sliced = {**one, "rows": 5000, "item_slices": 4}
    sizer = who.replace("_rows", "_workspace")
    need = c_int64()
    if who == "bpr_neighbors_rows":
        assert lib().bpr_neighbors_workspace(1, 5000, 8, 10, 0, 4, byref(need)) == 0
    elif who == "bpr_sample_rows":
        assert lib().bpr_sample_workspace(1, 5000, 8, 10, 4, 0, byref(need)) == 0
    else:
        assert getattr(lib(), sizer)(1, 5000, 8, 10, 4, byref(need)) == 0
    need = need.value
    assert need >= 320
    if who != "bpr_retrieve_rows":
        assert need == 320
    refused(call, sliced, f"{who}: workspace of 0 bytes, {need} needed ({sizer})")
    refused(call, {**sliced, "ws_bytes": need}, f"{who}: workspace of {need} bytes, {need} needed ({sizer})")  # NULL
    refused(call, {**sliced, "ws": 8, "ws_bytes": need - 1},
            f"{who}: workspace of {need - 1} bytes, {need} needed ({sizer})")
    refused(call, {**sliced, "ws": 4, "ws_bytes": need - 1},  # short and misaligned: short
            f"{who}: workspace of {need - 1} bytes, {need} needed ({sizer})")
    refused(call, {**sliced, "P": None}, NULL_TABLES[who])  # the tables come before the workspace
    assert call({**sliced, "n": 0}) == 0  # no rows: no workspace


def test_workspace_alignment_is_retrieve_s_and_sample_s_each_in_its_words():
    sliced = {**TOPK_GOOD, "n": 1, "rows": 5000, "item_slices": 4}
    need = c_int64()
    assert lib().bpr_retrieve_workspace(1, 5000, 8, 10, 4, byref(need)) == 0
    for ws in (4, 12, 1):
        refused(retrieve_rows, {**sliced, "ws": ws, "ws_bytes": need.value},
                "bpr_retrieve_rows: workspace must be 8-byte aligned")
        refused(sample_rows, {**sliced, "ws": ws, "ws_bytes": 320},
                "bpr_sample_rows: the workspace must be 8-byte aligned")
    # retrieve asks it of a workspace it does not need as well (no rows); sample does not
    assert lib().bpr_retrieve_workspace(0, 5000, 8, 10, 4, byref(need)) == 0 and need.value == 0
    refused(retrieve_rows, {**sliced, "n": 0, "ws": 4}, "bpr_retrieve_rows: workspace must be 8-byte aligned")
    assert retrieve_rows({**sliced, "n": 0, "ws": 8}) == 0
    assert sample_rows({**sliced, "n": 0, "ws": 4}) == 0
    # one slice, no log_z: sample needs no workspace and takes any
    assert sample_rows({**TOPK_GOOD, "n": 0, "ws": 4}) == 0


def test_rank_rows_null_tables_and_workspace():
    one = {**TOPK_GOOD, "n": 1}
    for name in ("P", "Q", "users"):
        refused(rank_rows, {**one, name: None}, "bpr_rank_rows: P, Q, users or tgt_indptr is NULL")
        assert rank_rows({**one, name: None, "n": 0}) == 0
    refused(rank_rows, {**one, "tptr": None}, "bpr_rank_rows: P, Q, users or tgt_indptr is NULL")
    refused(rank_rows, {**one, "P": None, "item_slices": 65},
            "bpr_rank_rows: item_slices must be 0 (choose) or in [1, 64]")
    sliced = {**one, "rows": 5000, "item_slices": 4}
    need = c_int64()
    assert lib().bpr_rank_workspace(1, 5000, 8, 4, byref(need)) == 0
    need = need.value
    assert need == 3 * 112 * 4
    refused(rank_rows, sliced, f"bpr_rank_rows: workspace of 0 bytes, {need} needed (bpr_rank_workspace)")
    refused(rank_rows, {**sliced, "ws": 8, "ws_bytes": need - 1},
            f"bpr_rank_rows: workspace of {need - 1} bytes, {need} needed (bpr_rank_workspace)")
    refused(rank_rows, {**sliced, "ws_bytes": need},
            f"bpr_rank_rows: workspace of {need} bytes, {need} needed (bpr_rank_workspace)")
    refused(rank_rows, {**sliced, "P": None}, "bpr_rank_rows: P, Q, users or tgt_indptr is NULL")
    assert rank_rows({**sliced, "n": 0}) == 0


# ---- rerank and diversify: layouts instead of slices, no workspace
RR_GOOD = dict(n=4, d=8, k=10, row_len=50, layout=0, I=100, P=1, Q=1, users=1, cptr=None, citems=1, sptr=None,
               sidx=None, cand_scores=None, items=1, scores=1)


def rerank_layout(a):
    lay = None if a.get("null_out") == "layout" else byref(c_int32())
    tile = None if a.get("null_out") == "tile" else byref(c_int32())
    return lib().bpr_rerank_layout(a["n"], a["d"], a["k"], a["row_len"], a["layout"], lay, tile)


def rerank_rows(a):
    return lib().bpr_rerank_rows(a["P"], a["Q"], None, a["I"], a["d"], a["users"], a["n"], a["cptr"], a["citems"],
                                 a["row_len"], a["sptr"], a["sidx"], a["k"], a["layout"], a["cand_scores"],
                                 a["items"], a["scores"], None)


RR_ENTRIES = {
    "bpr_rerank_layout": rerank_layout, "bpr_rerank_rows": rerank_rows,
    "bpr_test_rerank_plan": lambda a: hook("bpr_test_rerank_plan", a["n"], a["d"], a["k"], a["row_len"], a["layout"]),
}


@pytest.mark.parametrize("who", sorted(RR_ENTRIES))
def test_rerank_refuses_each_malformed_shape(who):
    call = RR_ENTRIES[who]
    if not who.endswith("_rows"):
        assert call(dict(RR_GOOD)) == 0
    n_msg, d_msg, k_msg = f"{who}: n must be >= 0", f"{who}: d must be in [1, 1024]", f"{who}: k must be in [0, 128]"
    len_msg = f"{who}: the list length must be >= 0"
    lay_msg = f"{who}: layout must be 0 (choose), 1 (wave per row) or 2 (workgroup per row)"
    for kw, message in [
        (dict(n=-1), n_msg), (dict(d=0), d_msg), (dict(d=1025), d_msg), (dict(k=-1), k_msg), (dict(k=129), k_msg),
        (dict(row_len=-1), len_msg), (dict(layout=-1), lay_msg), (dict(layout=3), lay_msg),
        (dict(n=-1, d=0), n_msg), (dict(d=0, k=129), d_msg), (dict(k=129, row_len=-1), k_msg),
        (dict(row_len=-1, layout=3), len_msg),
    ]:
        refused(call, {**RR_GOOD, **kw}, message)


def test_rerank_layout_and_rows_refusals():
    for which in ("layout", "tile"):
        refused(rerank_layout, {**RR_GOOD, "null_out": which}, "bpr_rerank_layout: layout_host or tile_host is NULL")
    refused(rerank_layout, {**RR_GOOD, "null_out": "tile", "n": -1},
            "bpr_rerank_layout: layout_host or tile_host is NULL")
    i_msg = "bpr_rerank_rows: I must be in [1, 2^31)"
    k0_msg = "bpr_rerank_rows: k == 0 asks for the candidate scores only: cand_scores_out is NULL"
    seen_msg = "bpr_rerank_rows: seen_indptr and seen_indices go together"
    null_msg = "bpr_rerank_rows: P, Q or users is NULL"
    for kw, message in [
        (dict(I=0), i_msg), (dict(I=B31), i_msg), (dict(I=0, layout=3),
                                                   "bpr_rerank_rows: layout must be 0 (choose), 1 (wave per row) or 2 "
                                                   "(workgroup per row)"),
        (dict(k=0), k0_msg), (dict(k=0, I=0), i_msg),
        (dict(sptr=1), seen_msg), (dict(sidx=1), seen_msg), (dict(sptr=1, k=0), k0_msg),
        (dict(P=None), null_msg), (dict(Q=None), null_msg), (dict(users=None), null_msg),
        (dict(P=None, sptr=1), seen_msg),
        (dict(citems=None), "bpr_rerank_rows: cand_items is NULL"),
        (dict(citems=None, cptr=1, row_len=0), "bpr_rerank_rows: cand_items is NULL"),
        (dict(citems=None, P=None), null_msg),
        (dict(items=None), "bpr_rerank_rows: items_out or scores_out is NULL"),
        (dict(scores=None), "bpr_rerank_rows: items_out or scores_out is NULL"),
        (dict(scores=None, citems=None), "bpr_rerank_rows: cand_items is NULL"),
    ]:
        refused(rerank_rows, {**RR_GOOD, **kw}, message)
    assert rerank_rows({**RR_GOOD, "n": 0, "P": None, "Q": None, "users": None, "citems": None}) == 0
    refused(rerank_rows, {**RR_GOOD, "n": 0, "sptr": 1}, seen_msg)  # (still validated)


DV_GOOD = dict(n=4, C=50, k=10, layout=0, Q=1, I=100, d=8, citems=1, cscores=1, lam=0.7, metric=1, scale=0, items=1,
               scores=1)


def diversify_layout(a):
    outs = [None if a.get("null_out") == i else byref(t()) for i, t in enumerate((c_int32, c_int32, c_int64))]
    return lib().bpr_diversify_layout(a["n"], a["C"], a["k"], a["layout"], *outs)


def diversify_rows(a):
    return lib().bpr_diversify_rows(a["Q"], a["I"], a["d"], a["citems"], a["cscores"], a["n"], a["C"], a["k"],
                                    a["lam"], a["metric"], a["scale"], a["layout"], a["items"], a["scores"], None, None)


DV_ENTRIES = {
    "bpr_diversify_layout": diversify_layout, "bpr_diversify_rows": diversify_rows,
    "bpr_test_diversify_plan": lambda a: hook("bpr_test_diversify_plan", a["n"], a["C"], a["k"], a["layout"]),
}


@pytest.mark.parametrize("who", sorted(DV_ENTRIES))
def test_diversify_refuses_each_malformed_shape(who):
    call = DV_ENTRIES[who]
    if not who.endswith("_rows"):
        assert call(dict(DV_GOOD)) == 0
    n_msg, c_msg, k_msg = f"{who}: n must be >= 0", f"{who}: C must be in [1, 128]", f"{who}: k must be in [0, 128]"
    lay_msg = f"{who}: layout must be 0 (choose) or 1 (workgroup per row)"
    for kw, message in [
        (dict(n=-1), n_msg), (dict(C=0), c_msg), (dict(C=129), c_msg), (dict(k=-1), k_msg), (dict(k=129), k_msg),
        (dict(layout=-1), lay_msg), (dict(layout=2), lay_msg),
        (dict(n=-1, C=0), n_msg), (dict(C=129, k=129), c_msg), (dict(k=-1, layout=2), k_msg),
    ]:
        refused(call, {**DV_GOOD, **kw}, message)


def test_diversify_layout_and_rows_refusals():
    for which in (0, 1, 2):
        refused(diversify_layout, {**DV_GOOD, "null_out": which},
                "bpr_diversify_layout: layout_host, cpad_host or lds_host is NULL")
    refused(diversify_layout, {**DV_GOOD, "null_out": 2, "C": 0},
            "bpr_diversify_layout: layout_host, cpad_host or lds_host is NULL")
    d_msg, i_msg = "bpr_diversify_rows: d must be in [1, 1024]", "bpr_diversify_rows: I must be in [1, 2^31)"
    lam_msg = "bpr_diversify_rows: lam must be in [0, 1]"
    metric_msg = "bpr_diversify_rows: metric must be BPR_SIM_DOT or BPR_SIM_COSINE"
    scale_msg = "bpr_diversify_rows: scale must be BPR_SCALE_NONE or BPR_SCALE_MINMAX"
    in_msg = "bpr_diversify_rows: Q, cand_items or cand_scores is NULL"
    out_msg = "bpr_diversify_rows: items_out or scores_out is NULL"
    for kw, message in [
        (dict(d=0), d_msg), (dict(d=1025), d_msg), (dict(I=0), i_msg), (dict(I=B31), i_msg),
        (dict(lam=-0.5), lam_msg), (dict(lam=1.5), lam_msg), (dict(lam=float("nan")), lam_msg),
        (dict(metric=-1), metric_msg), (dict(metric=2), metric_msg), (dict(scale=-1), scale_msg),
        (dict(scale=2), scale_msg),
        (dict(Q=None), in_msg), (dict(citems=None), in_msg), (dict(cscores=None), in_msg),
        (dict(items=None), out_msg), (dict(scores=None), out_msg),
        (dict(d=0, layout=2), "bpr_diversify_rows: layout must be 0 (choose) or 1 (workgroup per row)"),
        (dict(d=0, I=0), d_msg), (dict(I=0, lam=2.0), i_msg), (dict(lam=2.0, metric=2), lam_msg),
        (dict(metric=2, scale=2), metric_msg), (dict(scale=2, Q=None), scale_msg), (dict(Q=None, items=None), in_msg),
    ]:
        refused(diversify_rows, {**DV_GOOD, **kw}, message)
    for kw in (dict(n=0), dict(k=0)):
        assert diversify_rows({**DV_GOOD, **kw, "Q": None, "citems": None, "cscores": None, "items": None}) == 0
    refused(diversify_rows, {**DV_GOOD, "n": 0, "scale": 2}, scale_msg)  # (still validated)


# ---- the Python wrappers, as far as CPU tensors reach
def raises(kind, message, fn, *args, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind
    assert str(e.value) == message


def tables(U=8, I=16, d=4, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(U, d, generator=g).to(dtype), torch.randn(I, d, generator=g).to(dtype),
            torch.randn(I, generator=g).to(dtype))


USERS = torch.tensor([1, 2, 3], dtype=torch.int32)
NO_CPU = "; there is no CPU path in libbprcore"


def test_recommend_and_retrieve_on_the_cpu():
    from revisit_bpr.recommend import recommend
    from revisit_bpr.retrieve import retrieve

    P, Q, b = tables()
    for fn, name, kmax in ((recommend, "recommend", 128), (retrieve, "retrieve", 1024)):
        raises(ValueError, f"k = {kmax + 1}: {name} returns at most {kmax} items per user", fn, P, Q, b, USERS, kmax + 1)
        raises(ValueError, "k must be at least 1", fn, P, Q, b, USERS, 0)
        raises(ValueError, "k must be at least 1", fn, P, Q, b, USERS, -3)
        rocm = f"{name} needs the tables and the user list on a ROCm device" + NO_CPU
        raises(RuntimeError, rocm, fn, P, Q, b, USERS, 2)
        raises(RuntimeError, rocm, fn, P, Q, None, USERS, 2)
        # the device is asked for before the dtypes and the shapes
        raises(RuntimeError, rocm, fn, P.double(), Q[:, :3], b[:5], USERS.float(), 2,
               torch.zeros(3, dtype=torch.int32), None)


def test_sample_items_on_the_cpu():
    from revisit_bpr.sample import sample_items

    P, Q, b = tables()
    raises(ValueError, "k = 129: sample_items returns at most 128 items per user", sample_items, P, Q, b, USERS, 129)
    raises(ValueError, "k must be at least 1", sample_items, P, Q, b, USERS, 0)
    t_msg = "temperature must be finite and > 0 in float32, and so must 1 / temperature"
    for t in (0.0, -1.0, float("inf"), float("nan"), 1e-46, 1e39, 1e-39):
        raises(ValueError, t_msg, sample_items, P, Q, b, USERS, 2, temperature=t)
    for seed in (-1, 2 ** 64):
        raises(ValueError, "seed must be in [0, 2^64)", sample_items, P, Q, b, USERS, 2, seed=seed)
    raises(ValueError, "k must be at least 1", sample_items, P, Q, b, USERS, 0, temperature=0.0, seed=-1)
    raises(ValueError, t_msg, sample_items, P, Q, b, USERS, 2, temperature=0.0, seed=-1)
    rocm = "sample_items needs the tables and the user list on a ROCm device" + NO_CPU
    raises(RuntimeError, rocm, sample_items, P, Q, b, USERS, 2, seed=2 ** 64 - 1)
    raises(RuntimeError, rocm, sample_items, P.double(), Q, b, USERS.float(), 2)  # the device first


def test_neighbors_on_the_cpu():
    from revisit_bpr import similar

    P, Q, _ = tables()
    raises(ValueError, "k = 129: neighbors returns at most 128 ids per query", similar.neighbors, Q, Q, USERS, 129)
    raises(ValueError, "k must be at least 1", similar.neighbors, Q, Q, USERS, 0)
    metric_msg = "metric must be one of ['cosine', 'dot'], not 'l2'"
    raises(ValueError, metric_msg, similar.neighbors, Q, Q, USERS, 2, metric="l2")
    raises(ValueError, "first must be at least 0", similar.neighbors, Q, Q, USERS, 2, first=-1)
    raises(ValueError, "k must be at least 1", similar.neighbors, Q, Q, USERS, 0, metric="l2", first=-1)
    raises(ValueError, metric_msg, similar.neighbors, Q, Q, USERS, 2, metric="l2", first=-1)
    rocm = "neighbors needs the tables and the row list on a ROCm device; there is no CPU path in libbprcore"
    raises(RuntimeError, rocm, similar.neighbors, Q, Q, USERS, 2)
    raises(RuntimeError, rocm, similar.neighbors, Q.double(), P[:, :3], USERS, 2)
    raises(RuntimeError, rocm, similar.similar_items, Q, USERS, 2)
    raises(RuntimeError, rocm, similar.similar_users, P, USERS, 2, metric="dot")
    raises(ValueError, metric_msg, similar.similar_items, Q, USERS, 2, metric="l2")
    raises(ValueError, metric_msg, similar.workspace_bytes, 4, 100, 8, 10, "l2")


def test_rank_items_on_the_cpu():
    from revisit_bpr.ranks import rank_items

    P, Q, b = tables()
    tptr, titems = torch.tensor([0, 1, 2, 3]), torch.tensor([4, 5, 6], dtype=torch.int32)
    sptr, sidx = torch.zeros(9, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    share = "P [U, d] and Q [I, d] must share the embedding dim"
    seen_t = "seen_indptr must be int64 and seen_indices int32"
    for message, args, kw in [
        ("P must be float32", (P.double(), Q, b, USERS, tptr, titems), {}),
        ("Q must be float32", (P, Q.half(), b, USERS, tptr, titems), {}),
        ("item_bias must be float32", (P, Q, b.double(), USERS, tptr, titems), {}),
        ("P must be float32", (P.double(), Q.double(), b, USERS, tptr, titems), {}),
        (share, (P[0], Q, b, USERS, tptr, titems), {}), (share, (P, Q[0], b, USERS, tptr, titems), {}),
        (share, (P, Q[:, :3], b, USERS, tptr, titems), {}),
        ("item_bias must have one entry per item row", (P, Q, b[:5], USERS, tptr, titems), {}),
        ("users must be int32 or int64", (P, Q, b, USERS.float(), tptr, titems), {}),
        ("tgt_indptr must be int64 and tgt_items int32", (P, Q, b, USERS, tptr.int(), titems), {}),
        ("tgt_indptr must be int64 and tgt_items int32", (P, Q, b, USERS, tptr, titems.long()), {}),
        ("tgt_indptr must have n+1 entries", (P, Q, b, USERS, tptr[:3], titems), {}),
        ("tgt_indptr must have n+1 entries", (P, Q, b, USERS, tptr.reshape(2, 2), titems), {}),
        ("seen_indptr and seen_indices go together", (P, Q, b, USERS, tptr, titems, sptr), {}),
        ("seen_indptr and seen_indices go together", (P, Q, b, USERS, tptr, titems, None, sidx), {}),
        (seen_t, (P, Q, b, USERS, tptr, titems, sptr.int(), sidx), {}),
        (seen_t, (P, Q, b, USERS, tptr, titems, sptr, sidx.long()), {}),
        ("seen_indptr must have U+1 entries", (P, Q, b, USERS, tptr, titems, sptr[:8], sidx), {}),
        # two at once, in the wrapper's order
        ("item_bias must have one entry per item row", (P, Q, b[:5], USERS.float(), tptr, titems), {}),
        ("users must be int32 or int64", (P, Q, b, USERS.float(), tptr.int(), titems), {}),
        ("tgt_indptr must have n+1 entries", (P, Q, b, USERS, tptr[:3], titems, sptr), {}),
        (seen_t, (P, Q, b, USERS, tptr, titems, sptr[:8].int(), sidx), {}),
    ]:
        raises(ValueError, message, rank_items, *args, **kw)
    rocm = "rank_items needs the tables, the rows and the targets on a ROCm device" + NO_CPU
    raises(RuntimeError, rocm, rank_items, P, Q, b, USERS, tptr, titems)
    raises(RuntimeError, rocm, rank_items, P, Q, None, USERS.long(), tptr, titems, sptr, sidx)


def test_rerank_on_the_cpu():
    from revisit_bpr.rerank import rerank, score_candidates

    P, Q, b = tables()
    cand = torch.tensor([4, 5, 6, 7], dtype=torch.int32)
    cptr = torch.tensor([0, 1, 2, 4])
    sptr, sidx = torch.zeros(9, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    share = "P [U, d] and Q [I, d] must share the embedding dim"
    lay = "layout must be 0 (choose), 1 (wave per row) or 2 (workgroup per row)"
    seen_t = "seen_indptr must be int64 and seen_indices int32"
    for message, args, kw in [
        ("k = 129: rerank returns at most 128 items per row", (P, Q, b, USERS, cand, 129), {}),
        ("k must be at least 0", (P, Q, b, USERS, cand, -1), {}),
        ("k = 0 returns nothing without return_scores (score_candidates)", (P, Q, b, USERS, cand, 0), {}),
        (lay, (P, Q, b, USERS, cand, 2), dict(layout=3)), (lay, (P, Q, b, USERS, cand, 2), dict(layout=-1)),
        ("P must be float32", (P.double(), Q, b, USERS, cand, 2), {}),
        ("Q must be float32", (P, Q.double(), b, USERS, cand, 2), {}),
        ("item_bias must be float32", (P, Q, b.double(), USERS, cand, 2), {}),
        (share, (P, Q[:, :3], b, USERS, cand, 2), {}), (share, (P[0], Q, b, USERS, cand, 2), {}),
        ("item_bias must have one entry per item row", (P, Q, b[:5], USERS, cand, 2), {}),
        ("users must be int32 or int64", (P, Q, b, USERS.float(), cand, 2), {}),
        ("cand_items must be int32", (P, Q, b, USERS, cand.long(), 2), {}),
        ("cand_items without cand_indptr is ONE 1-D list shared by every row",
         (P, Q, b, USERS, cand.reshape(2, 2), 2), {}),
        ("cand_indptr must be int64", (P, Q, b, USERS, cand, 2, cptr.int()), {}),
        ("cand_indptr must have n+1 entries", (P, Q, b, USERS, cand, 2, cptr[:3]), {}),
        ("cand_indptr must have n+1 entries", (P, Q, b, USERS, cand, 2, cptr.reshape(2, 2)), {}),
        ("seen_indptr and seen_indices go together", (P, Q, b, USERS, cand, 2, None, sptr), {}),
        ("seen_indptr and seen_indices go together", (P, Q, b, USERS, cand, 2, None, None, sidx), {}),
        (seen_t, (P, Q, b, USERS, cand, 2, None, sptr.int(), sidx), {}),
        (seen_t, (P, Q, b, USERS, cand, 2, None, sptr, sidx.long()), {}),
        ("seen_indptr must have U+1 entries", (P, Q, b, USERS, cand, 2, None, sptr[:8], sidx), {}),
        # two at once, in the wrapper's order
        ("k = 129: rerank returns at most 128 items per row", (P, Q, b, USERS, cand, 129), dict(layout=3)),
        (lay, (P.double(), Q, b, USERS, cand, 2), dict(layout=3)),
        ("Q must be float32", (P, Q.double(), b[:5], USERS, cand, 2), {}),
        ("users must be int32 or int64", (P, Q, b, USERS.float(), cand.long(), 2), {}),
        ("cand_items must be int32", (P, Q, b, USERS, cand.long(), 2, cptr.int()), {}),
        ("cand_indptr must have n+1 entries", (P, Q, b, USERS, cand, 2, cptr[:3], sptr), {}),
    ]:
        raises(ValueError, message, rerank, *args, **kw)
    raises(ValueError, lay, score_candidates, P, Q, b, USERS, cand, layout=3)
    rocm = "rerank needs the tables, the user list and the candidates on a ROCm device" + NO_CPU
    raises(RuntimeError, rocm, rerank, P, Q, b, USERS, cand, 2)
    raises(RuntimeError, rocm, rerank, P, Q, None, USERS.long(), cand, 2, cptr, sptr, sidx)
    raises(RuntimeError, rocm, score_candidates, P, Q, b, USERS, cand)


def test_diversify_on_the_cpu():
    from revisit_bpr.diversify import diversify, intra_list_similarity, recommend_diverse

    P, Q, b = tables()
    ci = torch.tensor([[4, 5, 6], [7, 8, 9]], dtype=torch.int32)
    cs = torch.ones(2, 3)
    for message, args, kw in [
        ("k = 129: diversify returns at most 128 items per row", (Q, ci, cs, 129), {}),
        ("k must be at least 0", (Q, ci, cs, -1), {}),
        ("lam = 1.5: must be in [0, 1]", (Q, ci, cs, 2), dict(lam=1.5)),
        ("lam = -0.1: must be in [0, 1]", (Q, ci, cs, 2), dict(lam=-0.1)),
        ("lam = nan: must be in [0, 1]", (Q, ci, cs, 2), dict(lam=float("nan"))),
        ("unknown metric 'l2': 'cosine' or 'dot'", (Q, ci, cs, 2), dict(metric="l2")),
        ("unknown scale 'z': 'none' or 'minmax'", (Q, ci, cs, 2), dict(scale="z")),
        ("layout must be 0 (choose) or 1 (workgroup per row)", (Q, ci, cs, 2), dict(layout=2)),
        ("Q must be float32", (Q.double(), ci, cs, 2), {}),
        ("Q must be [I, d]", (Q[0], ci, cs, 2), {}),
        ("cand_items must be int32", (Q, ci.long(), cs, 2), {}),
        ("cand_scores must be float32", (Q, ci, cs.double(), 2), {}),
        ("cand_items and cand_scores must have the same shape", (Q, ci, cs[:, :2], 2), {}),
        ("cand_items must be [n, C], or 1-D for one row", (Q, ci[None], cs[None], 2), {}),
        ("C = 0: a pool holds 1 to 128 candidates", (Q, ci[:, :0], cs[:, :0], 2), {}),
        ("C = 129: a pool holds 1 to 128 candidates",
         (Q, torch.ones(2, 129, dtype=torch.int32), torch.ones(2, 129), 2), {}),
        # two at once, in the wrapper's order
        ("k must be at least 0", (Q, ci, cs, -1), dict(lam=2.0)),
        ("lam = 2.0: must be in [0, 1]", (Q, ci, cs, 2), dict(lam=2.0, metric="l2")),
        ("unknown metric 'l2': 'cosine' or 'dot'", (Q, ci, cs, 2), dict(metric="l2", scale="z")),
        ("unknown scale 'z': 'none' or 'minmax'", (Q, ci, cs, 2), dict(scale="z", layout=2)),
        ("layout must be 0 (choose) or 1 (workgroup per row)", (Q.double(), ci, cs, 2), dict(layout=2)),
        ("Q must be float32", (Q.double(), ci.long(), cs, 2), {}),
    ]:
        raises(ValueError, message, diversify, *args, **kw)
    rocm = "diversify needs the item table and the candidates on a ROCm device; there is no CPU path in libbprcore"
    raises(RuntimeError, rocm, diversify, Q, ci, cs, 2)
    raises(RuntimeError, rocm, diversify, Q, ci[0], cs[0], 0)
    raises(ValueError, "pool = 3 is shorter than k = 5", recommend_diverse, P, Q, b, USERS, 5, pool=3)
    raises(ValueError, "pool = 129: a pool holds at most 128 candidates", recommend_diverse, P, Q, b, USERS, 5, pool=129)
    raises(RuntimeError, "recommend needs the tables and the user list on a ROCm device" + NO_CPU,
           recommend_diverse, P, Q, b, USERS, 2, pool=4)
    raises(ValueError, "unknown metric 'l2': 'cosine' or 'dot'", intra_list_similarity, Q, ci, "l2")


def test_fold_in_tables_and_seen_csr_on_the_cpu():
    """fold-in takes `_table` and (fold_in_items) the seen-CSR check from the serving module: their words stay its own"""
    from revisit_bpr.foldin import fold_in
    from revisit_bpr.foldin_items import fold_in_items

    P, Q, b = tables()
    indptr, idx = torch.tensor([0, 1, 2]), torch.tensor([1, 2], dtype=torch.int32)
    sptr, sidx = torch.zeros(9, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    kw = dict(epochs=1, lr=0.1)
    raises(ValueError, "Q must be float32", fold_in, Q.double(), b, indptr, idx, **kw)
    raises(ValueError, "item_bias must be float32", fold_in, Q, b.double(), indptr, idx, **kw)
    raises(ValueError, "P must be float32", fold_in_items, P.double(), Q, b, indptr, idx, **kw)
    raises(ValueError, "Q must be float32", fold_in_items, P, Q.double(), b, indptr, idx, **kw)
    both = "seen_indptr and seen_indices must both be given or both be None"
    raises(ValueError, both, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr, **kw)
    raises(ValueError, both, fold_in_items, P, Q, b, indptr, idx, seen_indices=sidx, **kw)
    dt = "seen_indptr must be int64 and seen_indices int32"
    raises(ValueError, dt, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr.int(), seen_indices=sidx, **kw)
    raises(ValueError, dt, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr, seen_indices=sidx.long(), **kw)
    ln = "seen_indptr must have U+1 entries"
    raises(ValueError, ln, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr[:8], seen_indices=sidx, **kw)
    raises(ValueError, ln, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr.reshape(3, 3), seen_indices=sidx, **kw)
    raises(ValueError, dt, fold_in_items, P, Q, b, indptr, idx, seen_indptr=sptr[:8].int(), seen_indices=sidx, **kw)
    raises(ValueError, "indptr must be int64 and users int32", fold_in_items, P, Q, b, indptr.int(), idx,
           seen_indptr=sptr, **kw)  # the rows' CSR comes before the seen CSR


def test_the_sizing_wrappers_pass_the_library_s_refusal_on():
    from revisit_bpr import diversify, native, ranks, recommend, rerank, retrieve, sample, similar

    def refused_by_library(message, fn, *args):
        with pytest.raises(native.BprError) as e:
            fn(*args)
        assert str(e.value) == "libbprcore error -1: " + message and e.value.code == -1

    for mod, fam, kmax in ((recommend, "topk", 128), (retrieve, "retrieve", 1024), (sample, "sample", 128),
                           (similar, "neighbors", 128)):
        refused_by_library(f"bpr_{fam}_workspace: k must be in [1, {kmax}]", mod.workspace_bytes, 4, 100, 8, kmax + 1)
        refused_by_library(f"bpr_{fam}_slices: d must be in [1, 1024]", mod.slices, 4, 100, 0, 10)
        # (neighbors' default metric is the cosine: the norms of the 100 table rows and of no query)
        assert mod.workspace_bytes(0, 100, 8, 10) == (400 if mod is similar else 0) and mod.slices(4, 100, 8, 10) == 1
        assert isinstance(mod.workspace_bytes(4, 5000, 8, 10), int) and isinstance(mod.slices(1, 5000, 8, 10, 4), int)
        assert mod.slices(1, 5000, 8, 10, 4) == 4
    assert recommend.workspace_bytes(1, 5000, 8, 10, 4) == 320 == similar.workspace_bytes(1, 5000, 8, 10, "dot", 4)
    assert sample.workspace_bytes(1, 5000, 8, 10, 4, True) == 320 + 4 * 8 and sample.workspace_bytes(1, 5000, 8, 10, 4) == 320
    refused_by_library("bpr_rank_workspace: item_slices must be 0 (choose) or in [1, 64]", ranks.workspace_bytes,
                       4, 100, 8, 65)
    refused_by_library("bpr_rank_slices: n must be >= 0 and I in [1, 2^31)", ranks.slices, 4, 0, 8)
    assert ranks.workspace_bytes(1, 5000, 8, 4) == 3 * 112 * 4 and ranks.slices(1, 5000, 8, 4) == 4
    refused_by_library("bpr_rerank_layout: the list length must be >= 0", rerank.layout_of, 4, 8, 10, -1)
    refused_by_library("bpr_diversify_layout: C must be in [1, 128]", diversify.layout_of, 4, 0, 10)
    assert rerank.layout_of(4, 8, 10, 50, 2) == (2, 256) and diversify.layout_of(4, 50, 10)[0] == 1
