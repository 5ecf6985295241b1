"""A Python restatement of the MSM's plan (device/msm.hpp msm_cost,
msm_layout_groups) and of the predicate that picks the two-level counting sort
(msm.hip launch_msm_sort and its RS_* constants), written from the headers.

tests/test_msm_plan_cpu.py pins the model (the width transitions, the carry
constant) and proves that the sizes the GPU tests run reach every layout; the
GPU tests pin the model against the C++ by the sort kernel the timeline names
and by the work it books for k_msm_segments and k_msm_final.
The size lists of tests/test_gpu_msm_plans.py and tests/test_gpu_clean_close.py
live here so that the coverage proof and the GPU tests read the same lists."""

# device/msm.hpp
MSM_BITS = 127
MSM_SEG = 8
MSM_CH = 8
MSM_SCAN_ITEMS = 1024
MSM_WIN_ITEMS = 1024
# msm.hip
RS_PSH = 6
RS_SP = 4096
RS_MAX_NPG = 8192
RS_MIN_N = 4096
RS_IDX_MASK = 0x00FFFFFF


def msm_cost(n, c):
    nw = (MSM_BITS + c - 1) // c
    return float(nw) * (float(n) * 11.0 + float(1 << c) * 16.0)


def width_for(ptsg, maxc=16):
    """the window width msm_layout_groups takes for groups of ptsg points"""
    nvg = 2 * ptsg
    best = 4
    for c in range(5, maxc + 1):
        if msm_cost(nvg, c) < msm_cost(nvg, best):
            best = c
    return best


class Plan:
    """the fields of MsmPlan that msm_layout_groups sets"""

    def __init__(self, N, G, ptsg, maxc=16):
        c = width_for(ptsg, maxc)
        nw = (MSM_BITS + c - 1) // c
        lo = MSM_BITS // nw
        extra = MSM_BITS - lo * nw
        self.c, self.nw = c, nw
        self.widths, self.offs, self.bbase, self.sbase = [], [], [], []
        off = bb = sb = 0
        for w in range(nw):
            width = lo + (1 if w < extra else 0)
            nb = 1 << (width - 1)
            self.widths.append(width)
            self.offs.append(off)
            self.bbase.append(bb)
            self.sbase.append(sb)
            off += width
            bb += nb
            sb += (nb + MSM_SEG - 1) // MSM_SEG
        self.bits = off
        self.N, self.NV, self.G, self.ptsg = N, 2 * N, G, ptsg
        self.NBg, self.NSg = bb, sb
        self.NB, self.NS = G * bb, G * sb
        self.ch = MSM_CH
        self.NC = nw * (self.NV // self.ch + 1) + self.NB
        self.NBLK = (self.NB + MSM_SCAN_ITEMS - 1) // MSM_SCAN_ITEMS
        maxs = max(((1 << (w - 1)) + MSM_SEG - 1) // MSM_SEG for w in self.widths)
        self.WB = max(1, (maxs + MSM_WIN_ITEMS - 1) // MSM_WIN_ITEMS)

    def layout(self):
        """what names one of the window layouts: (c, nw, widths)"""
        return (self.c, self.nw, tuple(self.widths))

    def carry_constant(self):
        """C = sum_w (2^(width_w - 1) - 1) 2^off_w: k + C holds every window's
        signed digit as a bit field (launch_msm_sort's rc)"""
        return sum(((1 << (w - 1)) - 1) << o for w, o in zip(self.widths, self.offs))

    def two_level_sort(self, local_sort=True):
        """launch_msm_sort's predicate: k_rs_* (True) or k_msm_digits (False)"""
        m = (1 << RS_PSH) - 1
        rs = local_sort and self.N >= RS_MIN_N and self.NV <= RS_IDX_MASK and (self.NBg & m) == 0
        for w in range(self.nw):
            rs = rs and self.widths[w] > RS_PSH and (self.bbase[w] & m) == 0
        npg = self.NBg >> RS_PSH
        NP = self.G * npg
        sp = 2 * RS_SP if self.ptsg >= (1 << 21) else RS_SP
        spg = (self.ptsg + sp - 1) // sp
        S = self.G * spg
        return bool(rs and npg <= RS_MAX_NPG and self.ptsg > 0 and S * npg + 2 * NP <= self.nw * self.NV
                    and self.nw >= 4)

    def slices(self):
        """(slice size, points of the last slice of a group) of the two-level sort (rs_slice)"""
        sp = 2 * RS_SP if self.ptsg >= (1 << 21) else RS_SP
        spg = (self.ptsg + sp - 1) // sp
        size = (self.ptsg + spg - 1) // spg
        return size, self.ptsg - (spg - 1) * size


def layout(N, maxc=16):
    """msm_layout: one group"""
    return Plan(N, 1, N if N > 0 else 1, maxc)


def layout_groups(N, G, ptsg, maxc=16):
    return Plan(N, G, ptsg, maxc)


def sort_kernel(N, local_sort=True, maxc=16):
    """the sort kernel a standalone MSM of N points puts on its timeline"""
    return "k_rs_part" if layout(N, maxc).two_level_sort(local_sort) else "k_msm_digits"


def width_transitions(maxc=16, upto=1 << 18):
    """[(N, c)] for every N in [1, upto] whose width differs from N - 1's (N = 1
    first): an exhaustive scan, every cost an exact integer in a double.  The
    strict < of width_for keeps the narrowest width on a tie, as argmin does."""
    import numpy as np
    nv = 2.0 * np.arange(1, upto + 1, dtype=np.float64)
    cs = list(range(4, maxc + 1))
    cost = np.stack([float((MSM_BITS + c - 1) // c) * (nv * 11.0 + float(1 << c) * 16.0) for c in cs])
    width = np.asarray(cs)[np.argmin(cost, axis=0)]
    at = np.flatnonzero(np.diff(width)) + 1
    return [(1, int(width[0]))] + [(int(i) + 1, int(width[i])) for i in at]


def rp_npts(bits):
    """MSM points of one range proof in the batch check (2 log2(bits) + 5)"""
    return 2 * (bits.bit_length() - 1) + 5


# ---------------------------------------------------------------- the sizes run on the GPU
# tests/test_gpu_msm_plans.py: the standalone MSM
MSM_SIZES = [38, 39, 104, 105, 248, 249, 403, 404, 2234, 2235,
             4095, 4096, 4097, 8191, 8192, 8193,
             14894, 14895, 26810, 26811, 65537,
             154943, 154944, 166847, 166848]
# the true first sizes of c = 15 and c = 16 (and the sizes before them)
MSM_SIZES_EDGE = [154903, 154904, 166818, 166819]
# (N, FTS_MSM_SORT, FTS_MSM_MAXC) on contexts of their own
MSM_KNOB_CASES = [(4097, 0, 16), (26811, 0, 16), (65537, 1, 12), (4097, 1, 8)]

# tests/test_gpu_clean_close.py: proofs per honest pass
RP32_WORK_B = [1, 2, 3, 7, 8, 16, 17, 26, 27, 148, 149, 273, 274, 546, 547, 992, 993, 1787, 1788,
               10329, 10330, 11123, 11124]
RP32_WORK_B_EDGE = [10326, 10327, 11121, 11122]  # both sides of 154,904 and 166,819 points
RP32_LATENCY_B = [b for b in RP32_WORK_B if b <= 1788]


def bits_B(bits):
    """default-path pass sizes of bits 8, 16, 64: around the 4,096-point switch"""
    edge = -(-4096 // rp_npts(bits))
    return [1, edge - 1, edge, 1000]


COALESCED_SIZES = ([1, 7, 64, 200, 33, 128, 5, 90], [64] * 8)
