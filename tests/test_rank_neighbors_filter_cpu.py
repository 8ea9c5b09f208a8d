"""The item filter of `rank_items` / `evaluate_ranked` and of `neighbors` on a machine without a GPU:
  1. the `_from` functions of revisit-bpr_amd/csrc/bpr_item_filter.h (a lower bound that is a parameter) alone under
     the host sanitizers (tests/rank_neighbors_filter_plan_check.cpp) and through the library's hook
     `bpr_test_filter_words_from`, against numpy; the first = 1 case is the functions without the parameter;
  2. `evaluate_ranked`'s filtered arithmetic (`drop_filtered_targets`, `eligible_counts`, `ranked_metrics`) against a
     dense numpy computation on a toy problem, the ranks fed in as tensors;
  3. a numpy model of k_rank's seen cursors with tile skipping — four cursors per row, each keeping its residue class,
     one search across a run of skipped tiles — against the direct definition of every walked tile's mask;
  4. `pack_item_filter(first=)`, the wrappers' refusals and the C entries' refusals.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import filter_model as fm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
FIRSTS = (0, 1, 5, 33)
SIZES = (1, 31, 32, 33, 129, 300)
TILE = 128


def cases(N):
    """(name, uint32 words): random, all ones with the tail bits set, all zero, only row 0"""
    nw = fm.n_words(N)
    rng = np.random.default_rng(N)
    return [("random", rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)),   # tail bits set too
            ("all-ones-with-tail", np.full(nw, 0xFFFFFFFF, np.uint32)),
            ("all-zero", np.zeros(nw, np.uint32)),
            ("only-row-0", fm.pack(np.arange(N) == 0))]


def words_from(words, N, first):
    """numpy: the filter's words with the ids below `first` and at or past N cleared"""
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    ids = np.arange(bits.size)
    bits &= (ids >= first) & (ids < N)
    return np.packbits(bits, bitorder="little").view(np.uint32).copy(), bits


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/rank_neighbors_filter_plan_check.cpp under -fsanitize=address,undefined"""
    exe = tmp_path_factory.mktemp("rank_neighbors_filter") / "plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(ROOT / "tests" / "rank_neighbors_filter_plan_check.cpp"), "-o", str(exe)], check=True)
    return exe


# ---- 1. the header ---------------------------------------------------------------------------------------------------
def test_from_functions_alone_under_the_host_sanitizers(check_exe):
    r = subprocess.run([str(check_exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_filter_word_from_against_numpy(check_exe):
    todo = [(N, first, name, w) for N in SIZES for first in FIRSTS for name, w in cases(N)]
    text = "".join(f"{N} {first} " + " ".join(f"{int(x):x}" for x in w) + "\n" for N, first, _, w in todo)
    r = subprocess.run([str(check_exe), "-"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(todo)
    for line, (N, first, name, w) in zip(lines, todo):
        want, _ = words_from(w, N, first)
        assert [int(x, 16) for x in line.split()] == want.tolist(), (N, first, name)


@pytest.fixture(scope="module")
def hooks():
    from revisit_bpr import native

    lib = native.load()
    new = lib.bpr_test_filter_words_from
    new.restype = ctypes.c_int
    new.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 4
    old = lib.bpr_test_filter_tiles
    old.restype = ctypes.c_int
    old.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return new, old


def aligned_words(w):
    raw = np.zeros(len(w) + 4, np.uint32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + len(w)]
    out[:] = w
    return out


@pytest.mark.parametrize("N", SIZES)
def test_hook_gives_numpys_words_and_first_1_is_filter_word(hooks, N):
    new, old = hooks
    for name, w in cases(N):
        w = aligned_words(w)
        nw, tiles = len(w), len(w) // 4
        for first in FIRSTS:
            out, has = np.zeros(nw, np.uint32), np.full(32 * nw, 9, np.uint8)
            empty, nxt = np.full(tiles, 9, np.uint8), np.full(tiles, -1, np.int64)
            assert new(w.ctypes.data, N, first, out.ctypes.data, has.ctypes.data, empty.ctypes.data,
                       nxt.ctypes.data) == 0
            want, bits = words_from(w, N, first)
            what = (N, first, name)
            assert np.array_equal(out, want), what
            assert np.array_equal(has.astype(bool), bits), what
            live = bits.reshape(tiles, TILE).any(axis=1)
            assert np.array_equal(empty.astype(bool), ~live), what
            for t in range(tiles):
                later = np.flatnonzero(live[t:])
                assert nxt[t] == (t + later[0] if len(later) else tiles), what
            if first == 1:  # the functions without the parameter
                probe = np.arange(32 * nw, dtype=np.int64)
                pout, e1 = np.zeros((len(probe), 3), np.int64), np.full(tiles, 9, np.uint8)
                b = np.array([0, tiles], np.int64)
                got, cnt = np.zeros(tiles, np.int64), np.zeros(1, np.int64)
                assert old(w.ctypes.data, N, b.ctypes.data, 1, got.ctypes.data, cnt.ctypes.data, e1.ctypes.data,
                           probe.ctypes.data, len(probe), pout.ctypes.data) == 0
                assert np.array_equal(pout[:, 2].astype(bool), bits) and np.array_equal(e1, empty), what
                assert np.array_equal(fm.eligible_items(w, N), bits[:N]), what


# ---- 2. evaluate_ranked's arithmetic ---------------------------------------------------------------------------------
def toy():
    """E = 6 users over I = 40 items: scores with ties, seen rows, targets that are seen, item 0, filtered out"""
    rng = np.random.default_rng(5)
    I, E = 40, 6
    S = rng.integers(-4, 5, (E, I)).astype(np.float32) / 4      # many ties
    seen = [np.sort(rng.choice(np.arange(1, I), rng.integers(0, 12), replace=False)) for _ in range(E)]
    F = rng.random(I) < 0.6
    F[0] = True                                                  # item 0's bit means nothing
    tgts = []
    for u in range(E):
        t = list(rng.choice(np.arange(1, I), 7, replace=False))
        if u == 0:
            t.append(0)
        if len(seen[u]) and seen[u][0] not in t:
            t.append(int(seen[u][0]))                            # a seen target
        tgts.append(np.array(t, np.int32))
    tgts[3] = np.array([j for j in range(1, I) if not F[j]][:3], np.int32)   # every target filtered out
    tgts[4] = np.zeros(0, np.int32)                                          # no target at all
    return I, E, S, seen, F, tgts


def rank_model(s, elig, t):
    """rank_items' definition for target t of a row with scores s [I] and the eligible mask"""
    if t < 1 or t >= len(s) or not elig[t]:
        return -1, -1, -np.inf
    others = elig.copy()
    others[t] = False
    ids = np.flatnonzero(others)
    before = (s[ids] > s[t]) | ((s[ids] == s[t]) & (ids < t))
    return int(before.sum()), int((s[ids] >= s[t]).sum()), s[t]


def dense_metrics(I, S_u, elig, kept, ks, masked):
    """one user's metrics by the definitions, from the dense score row"""
    order = sorted(np.flatnonzero(elig), key=lambda j: (-S_u[j], j))
    pos_of = {j: p for p, j in enumerate(order)}
    n_pos = len(kept)
    uniq = sorted(set(int(t) for t in kept))
    got = sorted(pos_of[t] for t in uniq if t in pos_of)          # positions of the retrievable targets
    out = {"mrr": 1.0 / (1 + got[0]) if got else 0.0}
    for k in ks:
        kk = min(k, I)
        top = [p for p in got if p < kk]
        ideal = sum(1.0 / np.log2(i + 2.0) for i in range(min(n_pos, kk)))
        out[f"ndcg@{k}"] = sum(1.0 / np.log2(p + 2.0) for p in top) / ideal if n_pos else 0.0
        out[f"recall@{k}"] = len(top) / n_pos if n_pos else 0.0
        out[f"precision@{k}"] = len(top) / kk
        out[f"map@{k}"] = sum((i + 1) / (p + 1) for i, p in enumerate(top)) / min(n_pos, kk) if n_pos else 0.0
    if masked:
        s = np.where(elig, S_u.astype(np.float64), -1e13)
        pos = [t for t in uniq if 0 <= t < I]
        neg = np.setdiff1d(np.arange(I), pos)
    else:
        s = S_u.astype(np.float64)
        pos = [t for t in uniq if t in pos_of]
        neg = np.setdiff1d(np.flatnonzero(elig), pos)
    pairs = sum(int((s[p] > s[neg]).sum()) for p in pos)
    out["auc"] = pairs / (len(pos) * len(neg)) if len(pos) * len(neg) else float("nan")
    return out


@pytest.mark.parametrize("masked", [True, False], ids=["masked-negatives", "eligible-negatives"])
@pytest.mark.parametrize("filtered", [True, False], ids=["filter", "no-filter"])
def test_filtered_arithmetic_against_a_dense_computation(filtered, masked):
    from revisit_bpr.evaluation import drop_filtered_targets, eligible_counts, ranked_metrics
    from revisit_bpr.item_filter import pack_item_filter

    I, E, S, seen, F, tgts = toy()
    ks = (1, 3, 10, 100)
    f = pack_item_filter(I, mask=torch.from_numpy(F)) if filtered else None
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(t) for t in tgts])]), dtype=torch.int64)
    items = torch.from_numpy(np.concatenate(tgts).astype(np.int32))
    seen_indptr = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seen])]), dtype=torch.int64)
    seen_indices = torch.from_numpy(np.concatenate(seen).astype(np.int32))
    users = torch.arange(E, dtype=torch.int32)
    inF = F.copy() if filtered else np.ones(I, bool)
    inF[0] = False
    if filtered:
        ptr, items = drop_filtered_targets(ptr, items, I, f)
        kept = [np.array([t for t in row if t == 0 or inF[t]], np.int32) for row in tgts]
        assert items.tolist() == np.concatenate(kept).tolist()
        assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in kept])]).tolist()
        assert len(kept[3]) == 0
    else:
        kept = tgts
    elig = []
    for u in range(E):
        e = inF.copy()
        e[seen[u]] = False
        elig.append(e)
    n_elig = eligible_counts(I, users, seen_indptr, seen_indices, f)
    assert n_elig.tolist() == [int(e.sum()) for e in elig]
    assert eligible_counts(I, users, None, None, f).tolist() == [int(inF.sum())] * E
    triples = [rank_model(S[u], elig[u], int(t)) for u in range(E) for t in kept[u]]
    rank = torch.tensor([t[0] for t in triples], dtype=torch.int32)
    not_below = torch.tensor([t[1] for t in triples], dtype=torch.int32)
    score = torch.tensor([t[2] for t in triples], dtype=torch.float32)
    means, per = ranked_metrics(rank, not_below, score, ptr, items, I, n_elig, ks=ks, auc=True, extra=True,
                                per_user=True, masked_negatives=masked)
    want = [dense_metrics(I, S[u], elig[u], kept[u], ks, masked) for u in range(E)]
    assert set(per) == set(want[0])
    for key in per:
        w = np.array([x[key] for x in want])
        np.testing.assert_allclose(per[key].numpy(), w, rtol=1e-6, atol=0, equal_nan=True, err_msg=key)
        if not np.isnan(w).any():
            np.testing.assert_allclose(means[key], w.mean(), rtol=1e-6, err_msg=key)


# ---- 3. the seen cursors of k_rank's counting pass with tile skipping ------------------------------------------------
def walk_masks(seen, walked, first_tile):
    """The model: the row's sorted seen list, four cursors.  At the slice's first walked tile cursor c starts at
    lower_bound(first walked tile) + c; at every walked tile a cursor that is behind the tile jumps, by ONE search, to
    the first entry of its residue class (mod 4) at or past the tile, then sets the bits of its entries inside the
    tile, stepping by four.  -> {tile: 128-bit mask as a bool array}"""
    out = {}
    n = len(seen)
    base = int(np.searchsorted(seen, first_tile * TILE, side="left"))
    se = [base + c for c in range(4)]
    for t in walked:
        mask = np.zeros(TILE, bool)
        for c in range(4):
            nxt = seen[se[c]] if se[c] < n else 2 ** 31 - 1
            if nxt < t * TILE:
                at = int(np.searchsorted(seen, t * TILE, side="left"))
                assert at > se[c]
                se[c] += (at - se[c] + 3) & ~3
            while se[c] < n and seen[se[c]] < (t + 1) * TILE:
                li = seen[se[c]] - t * TILE
                assert li >= 0                       # the jump left nothing behind
                assert not mask[li]                  # and no two cursors share an entry
                mask[li] = True
                se[c] += 4
        out[t] = mask
    return out


def test_seen_cursors_across_skipped_tiles_give_every_walked_tiles_mask():
    rng = np.random.default_rng(11)
    tiles = 9
    I = tiles * TILE - 40
    for trial in range(300):
        live = rng.random(tiles) < rng.choice([0.2, 0.5, 0.9])
        if trial == 0:
            live[:] = [True, False, True, False, False, False, True, True, False]
        t0, t1 = sorted(rng.integers(0, tiles + 1, 2))
        walked = [t for t in range(t0, t1) if live[t]]
        if not walked:
            continue
        kind = trial % 5
        if kind == 0:
            seen = np.sort(rng.choice(np.arange(1, I), 4 * rng.integers(0, 40) + 1, replace=False))   # 4k + 1 entries
        elif kind == 1:   # ends inside a skipped run when there is one
            dead = [t for t in range(tiles) if not live[t]]
            hi = (dead[-1] + 1) * TILE - 3 if dead else I
            seen = np.sort(rng.choice(np.arange(1, max(hi, 3)), min(max(hi, 3) - 1, rng.integers(1, 150)), replace=False))
        elif kind == 2:
            seen = np.zeros(0, np.int64)
        elif kind == 3:
            seen = np.arange(1, I)                                                                     # everything
        else:
            seen = np.sort(rng.choice(np.arange(1, I), rng.integers(1, 600), replace=False))
        got = walk_masks(seen, walked, walked[0])
        for t in walked:
            want = np.zeros(TILE, bool)
            inside = seen[(seen >= t * TILE) & (seen < (t + 1) * TILE)] - t * TILE
            want[inside] = True
            assert np.array_equal(got[t], want), (trial, t)


# ---- 4. the Python and C surfaces ------------------------------------------------------------------------------------
def test_pack_first_clears_the_ids_below_it_and_the_default_changes_nothing():
    from revisit_bpr.item_filter import pack_item_filter, unpack_item_filter

    for N in SIZES:
        mask = np.ones(N, bool)
        plain = pack_item_filter(N, mask=torch.from_numpy(mask))
        assert np.array_equal(plain.numpy().view(np.uint32), fm.pack(mask))      # what it always was: bit 0 as given
        assert torch.equal(pack_item_filter(N, mask=torch.from_numpy(mask), first=0), plain)
        for first in (1, 5, 33):
            got = unpack_item_filter(pack_item_filter(N, mask=torch.from_numpy(mask), first=first), N).numpy()
            assert np.array_equal(got, np.arange(N) >= first), (N, first)
    with pytest.raises(ValueError, match="first"):
        pack_item_filter(10, allow=[1], first=-1)


def test_wrappers_refuse_a_malformed_filter_on_cpu_tensors():
    from revisit_bpr.evaluation import evaluate_ranked
    from revisit_bpr.ranks import rank_items
    from revisit_bpr.similar import neighbors, similar_items, similar_users

    P, Q, users = torch.zeros(4, 8), torch.zeros(300, 8), torch.zeros(2, dtype=torch.int32)
    ptr, tg = torch.tensor([0, 1, 2]), torch.ones(2, dtype=torch.int32)
    calls = [lambda f: rank_items(P, Q, None, users, ptr, tg, item_filter=f),
             lambda f: evaluate_ranked(P, Q, None, users, ptr, tg, None, None, item_filter=f),
             lambda f: neighbors(Q, Q, users, 5, item_filter=f),
             lambda f: similar_items(Q, users, 5, item_filter=f),
             lambda f: similar_users(Q, users, 5, item_filter=f)]
    good = torch.zeros(12, dtype=torch.int32)
    for call in calls:
        with pytest.raises(ValueError, match="packed int32"):
            call(good.to(torch.int64))
        with pytest.raises(ValueError, match="12 words for 300 items"):
            call(good[:8])
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros(24, dtype=torch.int32)[::2])
        with pytest.raises(RuntimeError, match="ROCm device"):
            call(good)


BAD = ctypes.c_void_p(0x1000)  # pointers that must never be read (there is no device here)


def test_c_entries_refuse_a_misaligned_filter_under_their_own_names():
    from revisit_bpr import native

    lib = native.load()

    def rank(f, n=4, slices=1, ws=None, ws_bytes=0):
        return lib.bpr_rank_rows_filtered(BAD, BAD, None, 300, 16, BAD, n, BAD, BAD, None, None, f, slices, ws,
                                          ws_bytes, BAD, BAD, BAD, None)

    def nbrs(f, n=4, k=5, first=0, ws=None, ws_bytes=0):
        return lib.bpr_neighbors_rows_filtered(BAD, BAD, 300, 16, BAD, n, None, first, native.SIM_DOT, f, k, 1, ws,
                                               ws_bytes, BAD, BAD, None)

    for name, call in (("bpr_rank_rows_filtered", rank), ("bpr_neighbors_rows_filtered", nbrs)):
        for off in (4, 8, 12, 1):
            assert call(ctypes.c_void_p(0x1000 + off)) == native.ERR_INVALID
            assert lib.bpr_last_error().decode() == f"{name}: item_filter must be 16-byte aligned"
        assert call(ctypes.c_void_p(0x1000), n=0, ws=BAD, ws_bytes=1 << 20) == native.OK
        assert call(None, n=0, ws=BAD, ws_bytes=1 << 20) == native.OK
    # the parents' refusals in the parents' order under the new names
    assert nbrs(ctypes.c_void_p(0x1004), k=0) == native.ERR_INVALID
    assert lib.bpr_last_error().decode().startswith("bpr_neighbors_rows_filtered: k must be in [1, ")
    assert nbrs(ctypes.c_void_p(0x1004), first=-1) == native.ERR_INVALID
    assert lib.bpr_last_error().decode() == "bpr_neighbors_rows_filtered: first must be >= 0"
    assert rank(ctypes.c_void_p(0x1000), slices=3) == native.ERR_INVALID
    assert lib.bpr_last_error().decode().startswith("bpr_rank_rows_filtered: workspace of 0 bytes, ")
    assert lib.bpr_last_error().decode().endswith("(bpr_rank_workspace)")
    assert rank(ctypes.c_void_p(0x1000), slices=99) == native.ERR_INVALID
    assert lib.bpr_last_error().decode().startswith("bpr_rank_rows_filtered: item_slices must be")


def test_header_and_ctypes_table_agree_on_the_new_entries():
    from revisit_bpr import native

    parent, new = native.SIGNATURES["bpr_rank_rows"][1], native.SIGNATURES["bpr_rank_rows_filtered"][1]
    assert new == parent[:11] + [ctypes.c_void_p] + parent[11:]      # behind seen_indices
    parent, new = native.SIGNATURES["bpr_neighbors_rows"][1], native.SIGNATURES["bpr_neighbors_rows_filtered"][1]
    assert new == parent[:9] + [ctypes.c_void_p] + parent[9:]        # behind metric
