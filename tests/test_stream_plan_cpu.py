"""The launch plan of a STREAM launch (revisit-bpr_amd/csrc/bpr_stream_plan.h: kernel, "seen?" structure, block, grid,
dynamic LDS, run length, and the LDS tier's rows and tail zones) on the CPU, through the library's test hook
`bpr_test_stream_plan` — integer arithmetic on the shape, no ctx and no GPU.

Expected values are worked out by hand from the rules (comments below) and from numbers the project records
(tests/test_gpu_hotlds.py: 158 LDS rows at the bench's shape; 2,075 blocks for an ML-20M chunk); the tail
zones are held to tests/hotlds_model.py, the model the GPU tests build their streams from."""
import ctypes

import numpy as np
import pytest

from hotlds_model import runs_of, zones

GIVEN, UNIFORM, ADAPTIVE = 0, 1, 2
CSR, BITMAP, LIST = 0, 1, 2  # the plan's `seen`; forcing one: bpr_set_tuning("seen") 1 | 2 | 3
PLAIN, LDS = 0, 1
FIELDS = ("kernel", "seen", "block", "grid", "shmem", "bm_words", "gpw_active", "run_len", "L", "tail1", "tail2")
MAX_GRID = 65536


def plan(n, I, d, sampler=GIVEN, cap=0, run_len=0, force_seen=0, cus=256, grid_cap=MAX_GRID, hot_H=0, asked=0,
         force=False, lds_block=0, tail=12, lds_allowed=True, occ=8):
    from revisit_bpr import native

    lib = native.load()
    fn = lib.bpr_test_stream_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    fn.restype = ctypes.c_int
    G = 32 if d <= 128 else 64  # bpr_bind_tables: lanes per triple, elements per lane
    per_lane = -(-d // G)
    E = (1 if per_lane <= 1 else 2 if per_lane <= 2 else 4) if G == 32 else (4 if per_lane <= 4 else 8 if per_lane <= 8 else 16)
    shape = (ctypes.c_int64 * 18)(n, I, d, G, E, sampler, cap, run_len, force_seen, cus, grid_cap, int(hot_H > 0), hot_H,
                                  asked, int(force), lds_block, tail, int(lds_allowed))
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn(shape, occ, out) == 0
    return dict(zip(FIELDS, out))


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8, 12, 30])
@pytest.mark.parametrize("gpw", [1, 2])
def test_tail_zones_are_the_models(L, gpw):
    """tail1 / tail2 of the LDS tier == hotlds_model.zones, over the sweep of test_hotlds_model_cpu.py's
    test_zones_partition_the_launch, and the kernel's runs on those tails cover [0, n) exactly.  (Small launches do
    not fill the chip: forced, as the GPU tests do; gpw = 1 is G = 64, one group per wave.)"""
    rng = np.random.default_rng(L * 10 + gpw)
    d = 32 if gpw == 2 else 256
    for n in [1, 7, 16, 199_168, 40_928] + [int(x) for x in rng.integers(1, 60_000, 6)]:
        for tail in (0, 12, 25, 50):
            p = plan(n, 700, d, run_len=L, hot_H=8, asked=8, force=True, tail=tail)
            assert p["kernel"] == LDS and p["L"] == 8 and p["run_len"] == L and p["gpw_active"] == gpw
            assert (p["tail1"], p["tail2"]) == zones(n, L, gpw, tail), (n, L, gpw, tail)
            runs, _, _ = runs_of(n, L, p["tail1"], p["tail2"])
            assert np.array_equal(np.concatenate([np.arange(a, b) for a, b in runs]), np.arange(n))


@pytest.mark.parametrize("tail", [12, 0])
def test_tail_zones_of_the_bench_launch(tail):
    n = 199_168
    p = plan(n, 20_109, 128, sampler=ADAPTIVE, hot_H=256, asked=8, tail=tail)
    assert p["kernel"] == LDS and p["L"] == 8 and p["run_len"] == 8 and p["gpw_active"] == 2
    assert (p["tail1"], p["tail2"]) == zones(n, 8, 2, tail)
    runs, _, _ = runs_of(n, 8, p["tail1"], p["tail2"])
    assert np.array_equal(np.concatenate([np.arange(a, b) for a, b in runs]), np.arange(n))


def test_bench_shape_takes_the_lds_tier_with_158_rows():
    """d = 128 (G = 32, E = 4), I = 20,109, adaptive, 256 rows asked, a hot block of 256, 256 CUs, no cap.
    Workgroup 1,024 (E <= 4) = 32 groups; a bitmap is (20,109 + 31) // 32 = 629 -> 632 words = 2,528 B, 32 of them
    80,896 B; the room is 160 KiB - (4 x 128 + 256 + 16 + 256) = 162,800 B, and 80,896 + 32,768 fits: bitmaps.
    Rows of 4 x 128 + 4 = 516 B: (162,800 - 80,896) // 516 = 158.  A workgroup holds 16 waves x 2 groups = 32 runs;
    199,168 triples are 24,896 runs of 8 >= 2 x 256 x 32 = 16,384: the launch fills the chip twice.  More than 256
    workgroups' worth of runs: one workgroup per CU."""
    p = plan(199_168, 20_109, 128, sampler=ADAPTIVE, hot_H=256, asked=256)
    assert p == dict(kernel=LDS, seen=BITMAP, block=1024, grid=256, shmem=32 * 2528 + 158 * 516, bm_words=632,
                     gpw_active=2, run_len=8, L=158, tail1=zones(199_168, 8, 2, 12)[0], tail2=zones(199_168, 8, 2, 12)[1])
    # the ctx's explicit run length is kept — not the plain kernel's pick, not 8
    assert plan(199_168, 20_109, 128, sampler=ADAPTIVE, hot_H=256, asked=256, run_len=5)["run_len"] == 5


@pytest.mark.parametrize("d", [32, 64, 128])
def test_lds_rows_as_the_gpu_tests_read_them(d):
    """What tests/test_gpu_hotlds.py asserts through stream_lds_rows(): I = 700, 20,000 triples (2,500 runs of 8: far
    from filling 256 CUs twice), 64 rows asked.  The bitmaps (24 words x 32 groups = 3 KB) leave room for > 300 rows."""
    n, I = 20_000, 700
    for sampler in (UNIFORM, ADAPTIVE):
        assert plan(n, I, d, sampler=sampler, hot_H=256, asked=64, force=True, run_len=8)["L"] == 64
        assert plan(n, I, d, sampler=sampler, hot_H=40, asked=64, force=True, run_len=8)["L"] == 40  # the block is all there is
        for kw in (dict(asked=0, force=True), dict(asked=64, force=True, lds_allowed=False), dict(asked=64, force=False),
                   dict(asked=64, force=True, hot_H=0), dict(asked=64, force=True, hot_H=7)):  # (fewer than 8 rows: no tier)
            p = plan(n, I, d, sampler=sampler, run_len=8, **{"hot_H": 256, **kw})
            assert p["kernel"] == PLAIN and p["L"] == 0 and p["tail1"] == 0 and p["tail2"] == 0 and p["block"] == 256, kw
    # E = 1 | 2 | 4: 1,024 threads = 32 groups of 2 runs per wave-pair -> 2 x 256 x 32 = 16,384 runs of 8 fill the chip twice
    assert plan(8 * 16_384, I, d, sampler=ADAPTIVE, hot_H=256, asked=64)["kernel"] == LDS
    assert plan(8 * 16_384 - 8, I, d, sampler=ADAPTIVE, hot_H=256, asked=64)["kernel"] == PLAIN
    # a forced CSR search has no LDS-tier instantiation (given negatives have no seen structure at all)
    assert plan(n, I, d, sampler=ADAPTIVE, hot_H=256, asked=64, force=True, force_seen=1)["kernel"] == PLAIN
    p = plan(n, I, d, sampler=GIVEN, hot_H=256, asked=64, force=True, force_seen=1)
    assert p["kernel"] == LDS and p["seen"] == CSR and p["bm_words"] == 0 and p["shmem"] == 64 * (4 * d + 4)
    # the staged lists instead of the bitmaps, forced: 512 words per group
    p = plan(n, I, d, sampler=ADAPTIVE, hot_H=256, asked=64, force=True, force_seen=3)
    assert p["seen"] == LIST and p["bm_words"] == 512 and p["shmem"] == 32 * 512 * 4 + 64 * (4 * d + 4)


def test_lds_tier_workgroup():
    """1,024 threads for E <= 4, 512 for E >= 8, capped by "lds_block", shrunk to whole waves under a cap."""
    kw = dict(sampler=GIVEN, hot_H=64, asked=8, force=True)
    assert plan(20_000, 700, 256, **kw)["block"] == 1024  # G = 64, E = 4
    assert plan(20_000, 700, 512, **kw)["block"] == 512   # E = 8
    assert plan(20_000, 700, 128, lds_block=256, **kw)["block"] == 256
    p = plan(20_000, 700, 128, cap=6, **kw)  # 6 groups of 32 lanes = 3 waves: one workgroup of 192 threads
    assert p["block"] == 192 and p["grid"] == 1
    # grid = workgroups for the runs, at most one per CU: 2,000 triples, tail 0 -> 250 runs of 8, 32 per workgroup
    assert plan(2_000, 700, 128, tail=0, **kw)["grid"] == 8
    assert plan(2_000, 700, 128, tail=0, cus=4, **kw)["grid"] == 4


def test_seen_structure():
    # d = 128: 8 groups per 256-thread block.  I = 65,536: 2,048 words x 4 B x 8 = 64 KiB exactly: fits
    p = plan(50_000, 65_536, 128, sampler=ADAPTIVE)
    assert (p["seen"], p["block"], p["bm_words"], p["shmem"]) == (BITMAP, 256, 2048, 65_536)
    # one item more: 2,049 -> 2,052 words (multiple of 4), 65,664 B: the staged lists, 512 words per group
    p = plan(50_000, 65_537, 128, sampler=UNIFORM)
    assert (p["seen"], p["block"], p["bm_words"], p["shmem"]) == (LIST, 256, 512, 8 * 512 * 4)
    # forced bitmap, I = 200,000, G = 32: 6,250 -> 6,252 words = 25,008 B per group; 8 groups 200,064 B and 4 groups
    # 100,032 B do not fit 64 KiB, 2 groups (one wave) 50,016 B do: the block halves twice
    p = plan(50_000, 200_000, 128, sampler=ADAPTIVE, force_seen=2)
    assert (p["seen"], p["block"], p["bm_words"], p["shmem"], p["gpw_active"]) == (BITMAP, 64, 6252, 50_016, 2)
    # ... and I = 300,000 (9,376 words, 75,008 B for one wave) does not fit at 64 either: the lists, at block 256 again
    p = plan(50_000, 300_000, 128, sampler=ADAPTIVE, force_seen=2)
    assert (p["seen"], p["block"], p["bm_words"]) == (LIST, 256, 512)
    # forced list / CSR at a size where the bitmap would fit
    assert plan(50_000, 700, 128, sampler=ADAPTIVE, force_seen=3)["seen"] == LIST
    p = plan(50_000, 700, 128, sampler=ADAPTIVE, force_seen=1)
    assert (p["seen"], p["bm_words"], p["shmem"]) == (CSR, 0, 0)
    # given negatives: nothing to look up, whatever is forced
    for force_seen in (0, 2, 3):
        p = plan(50_000, 700, 128, sampler=GIVEN, force_seen=force_seen)
        assert (p["seen"], p["block"], p["bm_words"], p["shmem"]) == (CSR, 256, 0, 0)


def test_caps_shrink_the_block_to_whole_waves():
    # max_inflight = 1 at G = 64: ONE wave walks the stream
    p = plan(1_000, 700, 256, cap=1)
    assert (p["block"], p["gpw_active"], p["grid"], p["run_len"]) == (64, 1, 1, 8)
    # ... at G = 32: one wave, one of its two groups at work
    p = plan(1_000, 700, 128, cap=1)
    assert (p["block"], p["gpw_active"], p["grid"]) == (64, 1, 1)
    p = plan(1_000, 700, 128, cap=3)  # 96 lanes -> two waves, both groups of a wave at work
    assert (p["block"], p["gpw_active"], p["grid"]) == (128, 2, 1)
    p = plan(1_000, 700, 128, cap=8)  # a full block
    assert (p["block"], p["gpw_active"], p["grid"]) == (256, 2, 1)


def test_run_length_follows_the_launch_size():
    """The rule test_stream_run_length_follows_the_launch_size checks on the GPU.  d = 128, occupancy 8 on 256 CUs:
    a 256-thread block holds 4 waves x 2 groups = 8 runs, the chip 8 x 256 x 8 = 16,384 at once."""
    kw = dict(sampler=ADAPTIVE, occ=8, cus=256)
    # 199,168 triples = 24,896 runs of 8 > 16,384: runs of 8; 3,112 blocks' worth at ~1.5 runs per group = 2,075 blocks
    p = plan(199_168, 20_109, 128, **kw)
    assert (p["kernel"], p["run_len"], p["grid"], p["block"], p["shmem"]) == (PLAIN, 8, 2075, 256, 8 * 632 * 4)
    # 40,000 triples = 5,000 runs of 8 < 16,384: the shortest of 4..8 that fits: 10,000 runs of 4 do; 1,250 blocks
    p = plan(40_000, 20_109, 128, **kw)
    assert (p["run_len"], p["grid"]) == (4, 1250)
    # 100,000 triples: 25,000 runs of 4, 20,000 of 5, 16,667 of 6 do not fit; 14,286 of 7 do; ceil(14,286 / 8) blocks
    p = plan(100_000, 20_109, 128, **kw)
    assert (p["run_len"], p["grid"]) == (7, 1786)
    # just below one residency in runs of 8: 16,383 runs of 8 -> no shorter run fits -> 8, no 1.5-runs packing
    p = plan(8 * 16_383, 20_109, 128, **kw)
    assert (p["run_len"], p["grid"]) == (8, 2048)
    # half the CUs (a masked stream): 8,192 runs at once; 10,000 runs of 4 no longer fit: 8,000 of 5 do
    p = plan(40_000, 20_109, 128, **{**kw, "cus": 128})
    assert (p["run_len"], p["grid"]) == (5, 1000)
    # an explicit run length is kept: 13,334 runs of 3
    p = plan(40_000, 20_109, 128, run_len=3, **kw)
    assert (p["run_len"], p["grid"]) == (3, 1667)
    # under a binding cap (1,024 groups < 5,000 runs of 8): 8; 1,024 groups = 128 blocks
    p = plan(40_000, 20_109, 128, cap=1024, **kw)
    assert (p["run_len"], p["grid"]) == (8, 128)
    # a cap that does not bind changes nothing
    p = plan(40_000, 20_109, 128, cap=1 << 20, **kw)
    assert (p["run_len"], p["grid"]) == (4, 1250)
    # BPR_MAX_BLOCKS caps the grid (in 256-thread blocks)
    assert plan(199_168, 20_109, 128, grid_cap=1000, **kw)["grid"] == 1000
