"""GPU: the standalone BN254 G1 MSM (fts_msm_stage / fts_msm_run) at every
window layout msm_layout_groups (device/msm.hpp) can produce, at both sides of
every width transition, and at the ragged sizes of the two-level counting sort
(msm.hip k_rs_*: slices of 4,096 points, the 4,095 / 4,096 / 4,097 switch from
k_msm_digits, a last chunk shorter than MSM_CH).

The batch check's MSM runs the same kernels, but there a wrong sum only sends
the pass to its fallback, which gives the right verdicts anyway; here the sum
is compared exactly with the oracle's (oracle/bn254.py, mathlib G1.Mul + Add):
with P_i = (i mod 4096 + 1) G, sum s_i P_i = (sum (s_i mod r)(i mod 4096 + 1)
mod r) G, one oracle multiplication per case.

tests/msm_plan.py restates the plan; tests/test_msm_plan_cpu.py proves that
these sizes reach all 11 layouts and both sorts.  Each case pins that model
against the C++: the timeline names the sort the model predicts, and the work
the timeline books for k_msm_segments and k_msm_final is that of the model's
buckets, windows and k_msm_windows blocks."""
import ctypes as C
import os
import random

import pytest

import msm_plan as mp
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

M = 4096
SPECIALS = [0, 1, bn.R - 1, bn.R, (1 << 256) - 1]
# device/rp_kernels.hpp: the timeline's work unit (field products) in u32 MADs
MADS_PER_MUL, COST_ADD, COST_DBL = 136.0, 16.0, 7.0


@pytest.fixture(scope="module")
def base():
    """64-byte encodings of (j + 1) G, j < 4096, by successive oracle additions"""
    out, acc = [], None
    for _ in range(M):
        acc = bn.g1_add(acc, bn.GEN)
        out.append(bn.g1_bytes(acc))
    return b"".join(out)


def _inputs(base, n, seed):
    """-> (points, scalars, expected sum) of an n-point case"""
    rng = random.Random(seed)
    raw = bytearray(rng.randbytes(32 * n))  # 256-bit scalars: some exceed r
    for q, i in enumerate(range(7, n, 1024)):
        raw[32 * i:32 * i + 32] = SPECIALS[q % len(SPECIALS)].to_bytes(32, "big")
    # the last point's scalar: random, non-zero mod r (a dropped tail changes the sum)
    raw[32 * (n - 1):32 * n] = rng.randrange(1, bn.R).to_bytes(32, "big")
    pts = bytearray((base * (-(-n // M)))[:64 * n])
    absent = {5, n - 2}
    for i in absent:
        pts[64 * i:64 * i + 64] = bytes(64)  # the identity
    total = 0
    for i in range(n):
        if i not in absent:
            total += (int.from_bytes(raw[32 * i:32 * i + 32], "big") % bn.R) * (i % M + 1)
    assert n - 1 not in absent and 5 < n - 2
    return bytes(pts), bytes(raw), bn.g1_bytes(bn.g1_mul(bn.GEN, total % bn.R))


def _timeline(st):
    """names (duplicates kept) and {name: MADs} of a staged MSM's last run"""
    from fts_gpu import _lib as L
    cap = 128
    names, ms, mads = (C.c_char_p * cap)(), (C.c_float * cap)(), (C.c_double * cap)()
    m = L.lib.fts_msm_timings(st._b, names, ms, mads, cap)
    assert 0 < m < cap, m  # nothing truncated
    return [names[i].decode() for i in range(m)], {names[i].decode(): mads[i] for i in range(m)}


def _check(pp, base, n, local_sort=True, maxc=16):
    pts, scs, want = _inputs(base, n, 0x9A5 + n)
    st = pp.stage_msm(pts, scs)
    try:
        got = st.run()
        assert got == want, n
        assert st.run() == got  # idempotent on the staged inputs
        names, mads = _timeline(st)
        plan = mp.layout(n, maxc)
        ran, other = ("k_rs_part", "k_msm_digits") if plan.two_level_sort(local_sort) else ("k_msm_digits", "k_rs_part")
        assert ran in names and other not in names, (n, names)
        # the plan the C++ laid out is the model's: buckets, windows, k_msm_windows blocks
        assert mads["k_msm_segments"] == plan.NB * 2 * COST_ADD * MADS_PER_MUL, (n, plan.c)
        final = sum(plan.offs) * COST_DBL + (plan.nw + 1) * (plan.WB + 1) * COST_ADD
        assert mads["k_msm_final"] == final * MADS_PER_MUL, (n, plan.c, plan.nw, plan.WB)
    finally:
        st.close()


@pytest.mark.parametrize("n", mp.MSM_SIZES + mp.MSM_SIZES_EDGE)
def test_msm_every_layout_and_ragged_size(gpu_pp, base, n):
    _check(gpu_pp(8), base, n)


@pytest.mark.parametrize("n,sort,maxc", mp.MSM_KNOB_CASES)
def test_msm_forced_sort_and_window_cap(pp_raw, base, n, sort, maxc):
    """FTS_MSM_SORT=0: k_msm_digits (device atomics + k_msm_scatter) at sizes the
    standalone MSM otherwise gives to the two-level sort; FTS_MSM_MAXC=12 / 8:
    narrower layouts at sizes where the default takes c = 13 / 10"""
    import fts_gpu
    env = dict(FTS_MSM_SORT=str(sort), FTS_MSM_MAXC=str(maxc))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pp = fts_gpu.PublicParams(pp_raw, bit_length=8, device=0, wide_bits=20)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        assert mp.layout(n, maxc).c == min(mp.layout(n).c, maxc)
        _check(pp, base, n, local_sort=bool(sort), maxc=maxc)
    finally:
        pp.close()
