"""The item filter on a machine without a GPU: revisit-bpr_amd/csrc/bpr_item_filter.h — the word and bit of an item,
"tile t is empty", "the next non-empty tile of [t, t1)" — compiled with the host compiler and held to the numpy
restatement of tests/filter_model.py, alone under the host sanitizers (tests/item_filter_plan_check.cpp) and through
the library's hook `bpr_test_filter_tiles`; `pack_item_filter` / `unpack_item_filter` on CPU tensors; the wrappers'
refusals of a malformed filter before any device is touched; and the C entries' refusal of a misaligned one.  No GPU."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import filter_model as fm

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
SIZES = (1, 127, 128, 129, 300, 4097)


def cases(I):
    """(name, uint32 words) — empty first, middle and last tile, all empty, all full, bits past I set on purpose"""
    nw, tiles = fm.n_words(I), fm.n_words(I) // fm.TILE_WORDS
    rng = np.random.default_rng(I)
    full = np.full(nw, 0xFFFFFFFF, np.uint32)
    out = [("all-empty", np.zeros(nw, np.uint32)),
           ("all-full-with-tail", full.copy()),                      # the tail bits and item 0's set on purpose
           ("all-full-packed", fm.pack(np.ones(I, bool))),
           ("random", fm.pack(rng.random(I) < 0.3)),
           ("sparse", fm.pack(rng.random(I) < 0.004)),
           ("only-item-0", fm.pack(np.arange(I) == 0))]
    tail = np.zeros(32 * nw, bool)
    tail[I:] = True
    out.append(("only-tail-bits", np.packbits(tail, bitorder="little").view(np.uint32).copy()))
    for name, t in (("first", 0), ("middle", tiles // 2), ("last", tiles - 1)):
        w = full.copy()
        w[fm.TILE_WORDS * t:fm.TILE_WORDS * (t + 1)] = 0
        out.append((f"{name}-tile-empty", w))
    return out


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/item_filter_plan_check.cpp under -fsanitize=address,undefined"""
    exe = tmp_path_factory.mktemp("item_filter") / "item_filter_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "item_filter_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    return exe


# ---- 1. the header, alone --------------------------------------------------------------------------------------------
def test_header_alone_under_the_host_sanitizers(check_exe):
    """bpr_item_filter.h is plain C++: the program's own sweep (every function against a loop over the items; the
    words in a heap block of exactly the filter's length) runs clean."""
    r = subprocess.run([str(check_exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_header_against_the_numpy_restatement(check_exe):
    todo = [(I, name, w) for I in SIZES for name, w in cases(I)]
    text = "".join(f"{I} " + " ".join(f"{int(x):x}" for x in w) + "\n" for I, _, w in todo)
    r = subprocess.run([str(check_exe), "-"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 4 * len(todo)
    for j, (I, name, w) in enumerate(todo):
        has, empty, nxt, at = (line.split(" ", 1)[1] if " " in line else "" for line in lines[4 * j:4 * j + 4])
        what = f"I={I} {name}"
        tiles = len(w) // fm.TILE_WORDS
        ok = np.zeros(32 * len(w) + 2, bool)        # ids -1 .. 32 * words
        ok[1:I + 1] = fm.eligible_items(w, I)
        assert has == "".join("1" if b else "0" for b in ok), what
        assert empty == "".join("1" if b else "0" for b in fm.empty_tiles(w, I)), what
        want = [fm.next_tile(w, I, t, t1) for t1 in range(tiles + 1) for t in range(t1 + 1)]
        assert [int(x) for x in nxt.split()] == want, what
        assert at.split() == [f"{i >> 5}:{i & 31}" for i in (0, 1, 31, 32, 33, 127, 128, I - 1)], what


# ---- 2. the same through the library ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook():
    from revisit_bpr import native

    fn = native.load().bpr_test_filter_tiles
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return fn


def aligned_words(w):
    """the words in a 16-byte aligned numpy buffer"""
    raw = np.zeros(len(w) + 4, np.uint32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + len(w)]
    out[:] = w
    assert out.ctypes.data % 16 == 0
    return out


@pytest.mark.parametrize("I", SIZES)
def test_hook_walks_the_non_empty_tiles_of_every_slice(hook, I):
    for name, w in cases(I):
        w = aligned_words(w)
        tiles = len(w) // fm.TILE_WORDS
        live = np.flatnonzero(~fm.empty_tiles(w, I))
        probe = np.array([-1, 0, 1, 31, 32, 127, 128, I - 1, I, 32 * len(w) - 1, 32 * len(w) + 5], np.int64)
        for slices in sorted({1, min(2, tiles), min(3, tiles), tiles}):
            bounds = np.array([tiles * s // slices for s in range(slices + 1)], np.int64)
            got, counts = np.full(tiles, -1, np.int64), np.full(slices, -1, np.int64)
            empty, pout = np.full(tiles, 9, np.uint8), np.zeros((len(probe), 3), np.int64)
            rc = hook(w.ctypes.data, I, bounds.ctypes.data, slices, got.ctypes.data, counts.ctypes.data,
                      empty.ctypes.data, probe.ctypes.data, len(probe), pout.ctypes.data)
            what = f"I={I} {name} slices={slices}"
            assert rc == 0, what
            assert np.array_equal(empty.astype(bool), fm.empty_tiles(w, I)), what
            assert counts.tolist() == [int(((live >= a) & (live < b)).sum()) for a, b in zip(bounds, bounds[1:])], what
            assert got[:len(live)].tolist() == live.tolist() and (got[len(live):] == -1).all(), what
            ok = fm.eligible_items(w, I)
            assert pout[:, 2].tolist() == [int(0 <= i < I and ok[i]) for i in probe], what
            assert np.array_equal(pout[:, 0], probe >> 5) and np.array_equal(pout[:, 1], probe & 31), what


def test_hook_refuses_a_misaligned_filter(hook):
    from revisit_bpr import native

    w = aligned_words(np.zeros(8, np.uint32))
    b = np.array([0, 1], np.int64)
    out = np.zeros(4, np.int64)
    assert hook(w.ctypes.data + 4, 128, b.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None, None, 0, None) == -1
    assert b"16-byte aligned" in native.load().bpr_last_error()


# ---- 3. pack / unpack ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", SIZES)
def test_pack_layout_length_tail_and_round_trip(I):
    from revisit_bpr.item_filter import filter_words, pack_item_filter, unpack_item_filter

    rng = np.random.default_rng(7 * I)
    mask = rng.random(I) < 0.5
    mask[I - 1] = True                                  # the last item, and with it bit 31 of some word at I = 128
    f = pack_item_filter(I, mask=torch.from_numpy(mask))
    assert f.dtype == torch.int32 and f.dim() == 1 and f.is_contiguous() and f.device.type == "cpu"
    assert f.numel() == filter_words(I) == fm.n_words(I) == 4 * -(-I // 128)
    assert np.array_equal(f.numpy().view(np.uint32), fm.pack(mask))     # the layout, tail zero included
    bits = np.unpackbits(f.numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:I].astype(bool), mask) and not bits[I:].any()
    assert np.array_equal(unpack_item_filter(f, I).numpy(), mask)


@pytest.mark.parametrize("I", SIZES)
def test_allow_is_the_complement_of_deny_and_duplicates_do_not_matter(I):
    from revisit_bpr.item_filter import pack_item_filter, unpack_item_filter

    rng = np.random.default_rng(11 * I)
    ids = np.unique(rng.integers(0, I, max(1, I // 3)))
    rest = np.setdiff1d(np.arange(I), ids)
    allow = pack_item_filter(I, allow=torch.from_numpy(ids))
    assert torch.equal(allow, pack_item_filter(I, deny=torch.from_numpy(rest)))
    assert np.array_equal(np.flatnonzero(unpack_item_filter(allow, I).numpy()), ids)
    twice = np.concatenate([ids, ids[::-1], ids[:1]])
    assert torch.equal(allow, pack_item_filter(I, allow=twice.tolist()))          # a list, with repeats
    assert torch.equal(pack_item_filter(I, deny=torch.from_numpy(ids)),
                       pack_item_filter(I, deny=torch.from_numpy(twice).to(torch.int32)))
    assert torch.equal(pack_item_filter(I, allow=[]), torch.zeros(fm.n_words(I), dtype=torch.int32))
    assert np.array_equal(pack_item_filter(I, deny=[]).numpy().view(np.uint32), fm.pack(np.ones(I, bool)))


def test_pack_refuses_bad_arguments():
    from revisit_bpr.item_filter import pack_item_filter, unpack_item_filter

    for bad in ([300], [-1], [5, 299, 300]):
        with pytest.raises(ValueError, match="out of range"):
            pack_item_filter(300, allow=bad)
        with pytest.raises(ValueError, match="out of range"):
            pack_item_filter(300, deny=bad)
    mask = torch.ones(300, dtype=torch.bool)
    for kw in ({}, {"allow": [1], "deny": [2]}, {"allow": [1], "mask": mask}, {"deny": [1], "mask": mask},
               {"allow": [1], "deny": [2], "mask": mask}):
        with pytest.raises(ValueError, match="exactly one"):
            pack_item_filter(300, **kw)
    for m in (torch.ones(299, dtype=torch.bool), torch.ones(300, dtype=torch.int32),
              torch.ones((300, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask must be bool"):
            pack_item_filter(300, mask=m)
    with pytest.raises(ValueError, match="integer item ids"):
        pack_item_filter(300, allow=torch.tensor([1.0]))
    with pytest.raises(ValueError):
        pack_item_filter(0, allow=[])
    with pytest.raises(ValueError, match="12 words"):
        unpack_item_filter(torch.zeros(8, dtype=torch.int32), 300)


# ---- 4. the wrappers refuse a malformed filter before the device is touched ------------------------------------------
def wrapper_calls():
    from revisit_bpr.diversify import recommend_diverse
    from revisit_bpr.recommend import recommend
    from revisit_bpr.retrieve import retrieve
    from revisit_bpr.sample import sample_items

    P, Q, users = torch.zeros(4, 8), torch.zeros(300, 8), torch.zeros(2, dtype=torch.int32)
    return [("recommend", lambda f: recommend(P, Q, None, users, 5, item_filter=f)),
            ("retrieve", lambda f: retrieve(P, Q, None, users, 5, item_filter=f)),
            ("sample_items", lambda f: sample_items(P, Q, None, users, 5, item_filter=f)),
            ("recommend_diverse", lambda f: recommend_diverse(P, Q, None, users, 5, pool=10, item_filter=f))]


@pytest.mark.parametrize("name, call", wrapper_calls(), ids=[n for n, _ in wrapper_calls()])
def test_wrappers_refuse_a_malformed_filter_on_cpu_tensors(name, call):
    good = torch.zeros(12, dtype=torch.int32)
    with pytest.raises(ValueError, match="packed int32"):
        call(good.to(torch.int64))
    with pytest.raises(ValueError, match="packed int32"):
        call(torch.ones(300, dtype=torch.bool))                      # a mask is not a packed filter
    with pytest.raises(ValueError, match="12 words for 300 items"):
        call(good[:8])                                               # short
    with pytest.raises(ValueError, match="12 words for 300 items"):
        call(good.reshape(3, 4))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(24, dtype=torch.int32)[::2])
    # a well-formed filter gets as far as the device refusal: there is no CPU path
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(good)
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(None)


# ---- 5. the C entries ------------------------------------------------------------------------------------------------
BAD = ctypes.c_void_p(0x1000)  # pointers that must never be read (there is no device here)


def c_calls(lib):
    """(name, call(filter pointer, **shape)) of the three _filtered entries"""
    def topk(name):
        fn = getattr(lib, name)
        return lambda f, k=5, n=4, ws=None, ws_bytes=0: fn(BAD, BAD, None, 300, 16, BAD, n, None, None, f, k, 1, ws,
                                                          ws_bytes, BAD, BAD, None)

    def sample(f, k=5, n=4, ws=None, ws_bytes=0):
        return lib.bpr_sample_rows_filtered(BAD, BAD, None, 300, 16, BAD, n, None, None, None, f, k, 1.0, 0, 1, ws,
                                            ws_bytes, BAD, BAD, None, None, None)
    return [("bpr_topk_rows_filtered", topk("bpr_topk_rows_filtered")),
            ("bpr_retrieve_rows_filtered", topk("bpr_retrieve_rows_filtered")),
            ("bpr_sample_rows_filtered", sample)]


def test_c_entries_refuse_a_misaligned_filter_under_their_own_names():
    from revisit_bpr import native

    lib = native.load()
    for name, call in c_calls(lib):
        for off in (4, 8, 12, 1):
            assert call(ctypes.c_void_p(0x1000 + off)) == native.ERR_INVALID
            assert lib.bpr_last_error().decode() == f"{name}: item_filter must be 16-byte aligned"
        # the parent's refusals, in the parent's order, under the new name: the shape comes first
        assert call(ctypes.c_void_p(0x1004), k=0) == native.ERR_INVALID
        assert lib.bpr_last_error().decode().startswith(f"{name}: k must be in [1, ")
        # n == 0 with an aligned filter, or with none, is BPR_OK and touches nothing
        assert call(ctypes.c_void_p(0x1000), n=0, ws=BAD, ws_bytes=1 << 20) == native.OK
        assert call(None, n=0, ws=BAD, ws_bytes=1 << 20) == native.OK
    # the workspace refusal names the entry and the parent's sizing call
    assert c_calls(lib)[1][1](ctypes.c_void_p(0x1000)) == native.ERR_INVALID
    assert lib.bpr_last_error().decode().startswith("bpr_retrieve_rows_filtered: workspace of 0 bytes, ")
    assert lib.bpr_last_error().decode().endswith("(bpr_retrieve_workspace)")


def test_header_and_ctypes_table_agree_on_the_new_entries():
    from revisit_bpr import native

    for fam in ("topk", "retrieve", "sample"):
        parent, new = native.SIGNATURES[f"bpr_{fam}_rows"][1], native.SIGNATURES[f"bpr_{fam}_rows_filtered"][1]
        at = 10 if fam == "sample" else 9       # behind seen_indices
        assert new == parent[:at] + [ctypes.c_void_p] + parent[at:]
