"""CPU: the MSM plan model (tests/msm_plan.py, a restatement of device/msm.hpp
msm_layout_groups and of msm.hip launch_msm_sort's predicate) and the coverage
proof of the GPU tests built on it.

The batch check hides an MSM error behind its fallback, and the standalone MSM
is where the MSM's value is observed exactly; so the sizes that
tests/test_gpu_msm_plans.py and tests/test_gpu_clean_close.py run must reach
every window layout the cost model can choose, both sorts, and the ragged
slices of the two-level sort.  This file asserts that they do, and fails when
a size leaves those lists."""
import pytest

import msm_plan as mp

# first N of every width (device/msm.hpp msm_cost): maxc = 16 (default), 12, 8
TABLE_16 = [(1, 4), (39, 5), (105, 6), (249, 7), (404, 8), (2235, 10), (8193, 11), (14895, 12), (26811, 13),
            (154904, 15), (166819, 16)]
NW_16 = {4: 32, 5: 26, 6: 22, 7: 19, 8: 16, 10: 13, 11: 12, 12: 11, 13: 10, 15: 9, 16: 8}
# what msm_layout (device/msm.hpp, compiled for the host) gives at the first N of
# every width: (N, c, nw, NB, NS, WB, NC)
CXX_16 = [(1, 4, 32, 252, 32, 1, 284), (39, 5, 26, 392, 49, 1, 652), (105, 6, 22, 624, 78, 1, 1218),
          (249, 7, 19, 1024, 128, 1, 2221), (404, 8, 16, 1984, 248, 1, 3616), (2235, 10, 13, 5888, 736, 1, 13155),
          (8193, 11, 12, 9728, 1216, 1, 34316), (14895, 12, 11, 17408, 2176, 1, 58372),
          (26811, 13, 10, 34816, 4352, 1, 101846), (154904, 15, 9, 81920, 10240, 2, 430463),
          (166819, 16, 8, 245760, 30720, 4, 579400)]
TABLE_12 = [t for t in TABLE_16 if t[1] <= 12]
TABLE_8 = [t for t in TABLE_16 if t[1] <= 8]

# the lists of the GPU tests, restated: a size removed there fails here
MSM_SIZES = [38, 39, 104, 105, 248, 249, 403, 404, 2234, 2235, 4095, 4096, 4097, 8191, 8192, 8193, 14894, 14895,
             26810, 26811, 65537, 154943, 154944, 166847, 166848]
# the two widest layouts start 40 and 29 points earlier than the sizes above assume
# (220 N + 1,310,720 = 198 N + 4,718,592 at N = 154,903.3; 198 N + 4,718,592 =
# 176 N + 8,388,608 at N = 166,818.9): their true first sizes and the ones before
MSM_SIZES_EDGE = [154903, 154904, 166818, 166819]
MSM_KNOB_CASES = [(4097, 0, 16), (26811, 0, 16), (65537, 1, 12), (4097, 1, 8)]
RP32_WORK_B = [1, 2, 3, 7, 8, 16, 17, 26, 27, 148, 149, 273, 274, 546, 547, 992, 993, 1787, 1788, 10329, 10330,
               11123, 11124]
RP32_WORK_B_EDGE = [10326, 10327, 11121, 11122]  # 15 B on both sides of 154,904 and of 166,819
BITS_B = {8: [1, 372, 373, 1000], 16: [1, 315, 316, 1000], 64: [1, 240, 241, 1000]}


@pytest.mark.parametrize("maxc,table", [(16, TABLE_16), (12, TABLE_12), (8, TABLE_8)])
def test_width_transitions(maxc, table):
    """every N up to 2^18: the width changes exactly at the table's sizes (widths 9
    and 14 are never the cheapest), and the scalar model agrees at both sides"""
    assert mp.width_transitions(maxc) == table
    for n, c in table:
        assert mp.width_for(n, maxc) == c
        if n > 1:
            assert mp.width_for(n - 1, maxc) < c
    assert mp.width_for(1 << 22, maxc) == table[-1][1]


def test_layout_fields():
    for n, c, nw, NB, NS, WB, NC in CXX_16:
        p = mp.layout(n)
        assert (p.c, p.nw, p.NB, p.NS, p.WB, p.NC) == (c, nw, NB, NS, WB, NC), n
    for n, c in TABLE_16:
        p = mp.layout(n)
        assert (p.c, p.nw) == (c, NW_16[c])
        assert p.bits == mp.MSM_BITS and sum(p.widths) == mp.MSM_BITS
        assert set(p.widths) <= {c, c - 1} and p.widths == sorted(p.widths, reverse=True)
        assert p.NBg == sum(1 << (w - 1) for w in p.widths) == p.NB
        assert p.NSg == sum(max(1, (1 << (w - 1)) // 8) for w in p.widths)
        assert p.NC == p.nw * (2 * n // 8 + 1) + p.NB
    # c = 15 is the one plan with two k_msm_windows blocks per window and with a
    # single window wider than the others
    wb2 = [c for n, c in TABLE_16 if mp.layout(n).WB == 2]
    assert wb2 == [15]
    assert mp.layout(154904).widths == mp.layout(154944).widths == [15] + [14] * 8
    assert all(mp.layout(n).WB == 1 for n, c in TABLE_16 if c != 15 and c != 16)
    assert mp.layout(166819).WB == 4 and mp.layout(166848).widths == [16] * 7 + [15]
    # a grouped plan takes its width from the group's points and scales the buckets
    g = mp.layout_groups(8 * 2600, 8, 2600)
    assert g.c == mp.layout(2600).c and g.NB == 8 * g.NBg and g.NS == 8 * g.NSg


@pytest.mark.parametrize("maxc", [16, 12, 8])
def test_carry_constant_below_2_126(maxc):
    """k + C < 2^127 for every GLV half k < 2^126 (bit 127 holds the sign on the device)"""
    for c in range(4, maxc + 1):
        # every width the loop of msm_layout_groups could return, chosen or not
        nw = (mp.MSM_BITS + c - 1) // c
        lo, extra = mp.MSM_BITS // nw, mp.MSM_BITS % nw
        off, C = 0, 0
        for w in range(nw):
            width = lo + (1 if w < extra else 0)
            C += ((1 << (width - 1)) - 1) << off
            off += width
        assert C < 1 << 126, c
    for n, _ in TABLE_16:
        assert mp.layout(n, maxc).carry_constant() < 1 << 126


def test_lists_are_the_ones_the_gpu_tests_run():
    assert mp.MSM_SIZES == MSM_SIZES and mp.MSM_SIZES_EDGE == MSM_SIZES_EDGE
    assert mp.MSM_KNOB_CASES == MSM_KNOB_CASES
    assert mp.RP32_WORK_B == RP32_WORK_B and mp.RP32_WORK_B_EDGE == RP32_WORK_B_EDGE
    assert mp.RP32_LATENCY_B == [b for b in RP32_WORK_B if b <= 1788]
    assert {bits: mp.bits_B(bits) for bits in (8, 16, 64)} == BITS_B
    assert [mp.rp_npts(b) for b in (8, 16, 32, 64)] == [11, 13, 15, 17]
    assert mp.COALESCED_SIZES == ([1, 7, 64, 200, 33, 128, 5, 90], [64] * 8)


def _layouts(sizes, maxc=16):
    return {mp.layout(n, maxc).layout() for n in sizes}


def test_sizes_reach_every_layout():
    every = {mp.layout(n).layout() for n, _ in TABLE_16}
    assert len(every) == 11
    # the standalone MSM: every layout, at the last size of one and the first of the next
    assert _layouts(MSM_SIZES) == every
    for n, c in TABLE_16[1:]:
        assert n in MSM_SIZES + MSM_SIZES_EDGE and n - 1 in MSM_SIZES + MSM_SIZES_EDGE, n
    # both WB == 2 sizes of the first list, and sizes of c = 13 beside them in the second
    assert [mp.layout(n).c for n in (154943, 154944, 166847, 166848)] == [15, 15, 16, 16]
    assert [mp.layout(n).c for n in MSM_SIZES_EDGE] == [13, 15, 15, 16]
    # the honest rp32 passes (15 points per proof): every layout on the work path,
    # and every layout below 2^15 points on the latency path
    work = [15 * b for b in RP32_WORK_B]
    assert _layouts(work) == every
    for (n0, c0), (n1, c1) in zip(TABLE_16, TABLE_16[1:]):
        below = [n for n in work if n0 <= n < n1]
        assert below and any(n >= n1 for n in work), (n0, n1)
    assert [mp.layout(15 * b).c for b in RP32_WORK_B_EDGE] == [13, 15, 15, 16]
    lat = [15 * b for b in mp.RP32_LATENCY_B]
    assert {l[0] for l in _layouts(lat)} == {4, 5, 6, 7, 8, 10, 11, 12, 13}
    # the knob cases: narrower caps give layouts of their own
    assert mp.layout(65537, 12).c == 12 and mp.layout(65537).c == 13
    assert mp.layout(4097, 8).c == 8 and mp.layout(4097).c == 10


def test_sizes_reach_both_sorts_and_ragged_slices():
    # below RS_MIN_N points: k_msm_digits whatever the plan
    assert all(not mp.layout(n).two_level_sort() for n in MSM_SIZES if n < 4096)
    assert not mp.layout(4095).two_level_sort() and mp.layout(4096).two_level_sort()
    # from 4,096 points: both values of the predicate
    big = [(n, 1, 16) for n in MSM_SIZES if n >= 4096] + MSM_KNOB_CASES
    seen = {mp.layout(n, maxc).two_level_sort(bool(sort)) for n, sort, maxc in big}
    assert seen == {True, False}
    assert all(mp.layout(n).two_level_sort() for n in MSM_SIZES if n >= 4096)
    assert [mp.sort_kernel(n, bool(s), m) for n, s, m in MSM_KNOB_CASES] == \
        ["k_msm_digits", "k_msm_digits", "k_rs_part", "k_rs_part"]
    # the two-level sort's slices (rs_slice): one full slice, a ragged last slice, a
    # last slice of one point, and a last chunk shorter than MSM_CH
    rs = [n for n in MSM_SIZES if n >= 4096]
    last = {n: mp.layout(n).slices() for n in rs}
    assert last[4096] == (4096, 4096)
    assert any(size != tail for size, tail in last.values())
    assert any(n % 4096 for n in rs) and any(n % 4096 == 0 for n in rs)
    assert any(n % mp.MSM_CH for n in rs) and any((2 * n) % mp.MSM_CH for n in rs)
    # honest passes: both sides of the switch on every bit length
    for bits, bs in [(32, RP32_WORK_B)] + sorted(BITS_B.items()):
        npts = mp.rp_npts(bits)
        assert any(b * npts < 4096 for b in bs) and any(b * npts >= 4096 for b in bs), bits
        edge = -(-4096 // npts)
        assert edge - 1 in bs and edge in bs, bits
        assert not mp.layout((edge - 1) * npts).two_level_sort() and mp.layout(edge * npts).two_level_sort()
    # the coalesced passes' per-caller-batch plan (FTS_MAIN_GROUPS=1): 8 groups padded to
    # the largest batch
    for sizes in mp.COALESCED_SIZES:
        gs = max(sizes) * mp.rp_npts(16)
        g = mp.layout_groups(len(sizes) * gs, len(sizes), gs)
        assert g.G == 8 and g.N >= 4096
