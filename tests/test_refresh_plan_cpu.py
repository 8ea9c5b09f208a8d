"""The sorter plan of a snapshot refresh (revisit-bpr_amd/csrc/bpr_refresh_plan.h: route, workgroups per column,
kernel instantiations, fallback) on the CPU, through the library's test hook `bpr_test_refresh_plan` — integer rules on
the shape and the tuning knobs, no ctx and no GPU.  Expected values are worked out by hand from the rules (comments)."""
import ctypes

import pytest

RADIX, BINNED, BINNED_SPLIT, PARTIAL, DEVICE = range(5)  # RefreshRoute
FB_NONE, FB_FLAGGED, FB_RADIX = range(3)                 # RefreshFallback
FIELDS = ("route", "sub", "len", "g", "sitems", "items", "fallback", "fb_items", "wide", "partial")


def plan(I, d=128, split=False, part=False, binned_sort=1, binned_split=0, refresh_sub=0, partial_snapshot=0,
         no_fast=False):
    from revisit_bpr import native

    fn = native.load().bpr_test_refresh_plan
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    fn.restype = ctypes.c_int
    shape = (ctypes.c_int64 * 9)(I, d, int(split), int(part), binned_sort, binned_split, refresh_sub, partial_snapshot,
                                 int(no_fast))
    out = (ctypes.c_int64 * len(FIELDS))()
    assert fn(shape, out) == 0
    return dict(zip(FIELDS, out))


# ---- pins of the rules as they were before the 17-bit range

def test_ml20m_is_one_binned_workgroup_per_column():
    """I = 20,109 <= 20,480: G = 1, k_sort_binned; 20,109 -> 20,112 keys = 20 per thread (19.6 -> ITEMS 20)."""
    p = plan(20109)
    assert (p["route"], p["g"], p["items"], p["sub"], p["len"]) == (BINNED, 1, 20, 1, 20112)
    assert not p["wide"] and not p["partial"]


def test_msd_is_three_workgroups_of_sixteen():
    """I = 41,141: G = (41,141 x 106 / 100 + 20,479) / 20,480 = (43,609 + 20,479) / 20,480 = 3; a stretch needs
    13,713 x 106 / 100 + 64 = 14,535 + 64 = 14,599 <= 16,384: SITEMS 16.  The column does not fit one radix workgroup
    (36,864): a flagged column goes to 2 radix workgroups of 20,576 keys (ceil(41,141 / 2) = 20,571 -> 16 | 20,576;
    21 per thread -> ITEMS 24) + one merge."""
    p = plan(41141)
    assert (p["route"], p["g"], p["sitems"], p["wide"]) == (BINNED_SPLIT, 3, 16, 0)
    assert (p["fallback"], p["sub"], p["len"], p["fb_items"]) == (FB_RADIX, 2, 20576, 24)


def test_last_16_bit_size_is_four_workgroups():
    """I = 65,535: (69,467 + 20,479) / 20,480 = 4; 16,383 x 106 / 100 + 64 = 17,429 -> SITEMS 20."""
    p = plan(65535)
    assert (p["route"], p["g"], p["sitems"], p["wide"]) == (BINNED_SPLIT, 4, 20, 0)
    assert (p["fallback"], p["sub"], p["len"], p["fb_items"]) == (FB_RADIX, 2, 32768, 36)


def test_split_binned_up_to_one_radix_workgroup_falls_back_to_k_sort_flagged():
    """I = 30,001 <= 36,864: G = (31,801 + 20,479) / 20,480 = 2, 15,000 x 1.06 + 64 = 15,964 -> 16; a flagged column
    fits one workgroup: sub = 1, k_sort_flagged<36> (30,016 keys: 30 per thread)."""
    p = plan(30001)
    assert (p["route"], p["g"], p["sitems"]) == (BINNED_SPLIT, 2, 16)
    assert (p["fallback"], p["sub"], p["fb_items"]) == (FB_FLAGGED, 1, 36)


def test_small_tables_and_the_switches_take_the_radix_sort():
    """Below 2,048 items, with binned_sort 0, with BPR_NO_FAST_REFRESH... the radix family."""
    p = plan(2047)  # d = 128: 128 x 1 < 256 but 2,047 / 2 < 5,000: whole columns; 2,048 keys -> ITEMS 6
    assert (p["route"], p["g"], p["sub"], p["items"]) == (RADIX, 0, 1, 6)
    p = plan(20109, binned_sort=0)  # 128 x 1 < 256 and 20,109 / 2 >= 5,000 -> 2; 256 = 256 stops it; 10,064 keys -> 10
    assert (p["route"], p["g"], p["sub"], p["len"], p["items"]) == (RADIX, 0, 2, 10064, 10)
    p = plan(20109, no_fast=True)  # no in-LDS sort at all: the device-wide one
    assert (p["route"], p["g"]) == (DEVICE, 0)


@pytest.mark.parametrize("sub", [2, 4])
def test_refresh_sub_forces_the_radix_split(sub):
    p = plan(20109, refresh_sub=sub)
    assert (p["route"], p["g"], p["sub"]) == (RADIX, 0, sub)
    assert p["len"] == {2: 10064, 4: 5040}[sub]  # ceil(20,109 / sub) rounded up to 16


def test_150k_items_take_the_device_wide_sort():
    """I = 150,000: four workgroups would hold 37,500 > 36,864 keys each."""
    p = plan(150000)
    assert (p["route"], p["g"], p["sub"], p["items"]) == (DEVICE, 0, 4, 0)


def test_split_refresh_with_partial_snapshot_sorts_partially():
    """_begin with partial_snapshot on, I <= 65,535, the column in one workgroup of <= 24,576 keys: k_sort_partial."""
    p = plan(20109, split=True, partial_snapshot=1)
    assert (p["route"], p["partial"], p["g"], p["items"]) == (PARTIAL, 1, 0, 20)
    # ... and where no partial order exists for the shape (41,141 does not fit one workgroup) the clause still keeps the
    # binned sort off, as before: the split radix sort with whole-as-possible columns (sub = 2)
    p = plan(41141, split=True, partial_snapshot=1)
    assert (p["route"], p["partial"], p["g"], p["sub"]) == (RADIX, 0, 0, 2)
    # a sharded refresh (_part) never sorts partially
    p = plan(20109, part=True, partial_snapshot=1)
    assert (p["route"], p["partial"]) == (BINNED, 0)


def test_forced_binned_split_on_a_small_table():
    """binned_split 3 at 20,108 items (tests/test_gpu_parity.py): 6,702 x 1.06 + 64 = 7,168 <= 8,192 -> SITEMS 8;
    binned_split 1 past 20,480 items cannot be honoured: the radix sort."""
    p = plan(20108, binned_split=3)
    assert (p["route"], p["g"], p["sitems"], p["fallback"], p["sub"]) == (BINNED_SPLIT, 3, 8, FB_FLAGGED, 1)
    p = plan(41141, binned_split=1)
    assert (p["route"], p["g"]) == (RADIX, 0)


# ---- 65,536 .. 131,071 items: 17-bit ids

@pytest.mark.parametrize("I,G,sitems,sub", [
    (65536, 4, 20, 2),    # (69,468 + 20,479) / 20,480 = 4; 16,384 x 1.06 + 64 = 17,431 -> 20; 2 x 36,864 holds the column
    (92090, 5, 20, 4),    # (97,615 + 20,479) / 20,480 = 5; 18,418 x 1.06 + 64 = 19,587 -> 20; 46,045 > 36,864 -> sub 4
    (131071, 7, 20, 4),   # (138,935 + 20,479) / 20,480 = 7; 18,724 x 1.06 + 64 = 19,911 -> 20
])
def test_forced_binned_split_reaches_the_wide_kernel(I, G, sitems, sub):
    """With binned_split forced the route is the split binned sort with 17-bit ids, G x CAP covers I x 1.06, and a
    flagged column goes to the filtered split radix sort + merge (d = 128: no extra split for idle CUs)."""
    for ask in (2, G, G + 1, 16):
        p = plan(I, binned_split=ask)
        assert (p["route"], p["wide"], p["fallback"], p["sub"]) == (BINNED_SPLIT, 1, FB_RADIX, sub), ask
        assert p["g"] == max(ask, G) and p["g"] * p["sitems"] * 1024 >= I * 1.06  # (too small an ask is raised)
        assert (I // p["g"]) * 106 // 100 + 64 <= p["sitems"] * 1024
        if ask <= G:
            assert p["sitems"] == sitems
    assert p["fb_items"] in (24, 36) and p["len"] * sub >= I


def test_131072_items_are_as_before():
    """One past 17 bits, forced or not: four radix workgroups of 32,768 keys (ITEMS 36) + two merge levels."""
    for ask in (0, 8):
        p = plan(131072, binned_split=ask)
        assert (p["route"], p["g"], p["wide"], p["sub"], p["len"], p["items"]) == (RADIX, 0, 0, 4, 32768, 36)


def test_begin_at_yelp_size_is_not_blocked_by_the_partial_clause():
    """No partial snapshot exists past 65,535 items, so partial_snapshot = 1 must not keep the side-stream refresh
    (_begin / _commit) off the binned route there."""
    on = plan(92090, split=True, partial_snapshot=1, binned_split=5)
    off = plan(92090, split=True, partial_snapshot=0, binned_split=5)
    assert on == off and on["route"] == BINNED_SPLIT and on["partial"] == 0 and on["g"] == 5
    assert plan(92090, split=True, partial_snapshot=1) == plan(92090, split=True, partial_snapshot=0)


def test_default_route_at_the_new_sizes():
    """The automatic choice extends to a size only where the new route was MEASURED faster than radix + merge with
    ranges that do not overlap.  No such measurement exists yet for 65,536 .. 131,071 items, so the
    default there stays what it was — the radix sort + merge, sub = 2 up to 73,728 items and 4 beyond — and the wide
    kernel is reached through `binned_split` (REFRESH_BINNED_AUTO_MAX = 65,535)."""
    for I, sub in ((65536, 2), (92090, 4), (131071, 4)):
        p = plan(I)
        assert (p["route"], p["g"], p["wide"], p["sub"]) == (RADIX, 0, 0, sub), I
        assert plan(I, binned_sort=0) == p
