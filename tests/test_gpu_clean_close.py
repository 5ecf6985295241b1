"""GPU: honest passes close the batch check.

rp_finish (api_rp.cpp) reads a random linear combination that does not close as
"some proof is bad" and then decides every proof by the single-fault locator,
the group test and the per-proof final equations, whose verdicts are the
reference's whatever the main path computed.  So an error in k_rlc_prep's
weights, the column sums, the fixed-base column products, the pass's MSM, the
`sel` gather of the per-caller-batch check or a ragged tail of the sort leaves
every verdict test green: the library merely runs every pass twice.

Here every pass is honest, and beside the verdicts (all accepted) each case
asserts the pass counters (fts_debug_pass_stats): at least one pass finished,
none whose combination did not close, no locator hit, no proof handed to the
per-proof equations.  An honest pass that falls back is the failure this file
exists to catch: no case is skipped or excluded.

The pass sizes (tests/msm_plan.py) put the pass's MSM at every window layout
and on both sides of the 4,096-point switch between the two sorts
(tests/test_msm_plan_cpu.py proves it), on both com paths, at every bit
length, in coalesced passes with one combination per pass and per caller
batch, and in action calls."""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest

import msm_plan as mp
from oracle import bn254 as bn, zkat

pytestmark = pytest.mark.gpu

STATUS_OF = {None: 0, "invalid range proof": 3, "invalid IPA": 6, "invalid range proof: nil elements": 2,
             "invalid IPA proof: nil elements": 4, "invalid IPA proof": 5}


def _ctx(pp_raw, bits, **env):
    """a context of its own (20-bit wide tables: the smaller footprint beside the
    session's contexts) created under the given FTS_* variables"""
    import fts_gpu
    env = {k: str(v) for k, v in env.items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fts_gpu.PublicParams(pp_raw, bit_length=bits, device=0, wide_bits=20)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_WORK, _PROOFS = {}, {}
N_PROOFS = {8: 1000, 16: 1000, 32: max(mp.RP32_WORK_B + mp.RP32_WORK_B_EDGE), 64: 1000}


@pytest.fixture(scope="module")
def work_pp(pp_raw):
    """factory: one work-path context (FTS_COM_FIXED_MAX=0, one lane) per bit length"""
    def get(bits):
        if bits not in _WORK:
            _WORK[bits] = _ctx(pp_raw, bits, FTS_COM_FIXED_MAX=0, FTS_LANES=1)
        return _WORK[bits]
    yield get
    for pp in _WORK.values():
        pp.close()
    _WORK.clear()
    _PROOFS.clear()


def _honest(pp, bits):
    """honest proofs of the bit length, made once on the device and shared (every
    case verifies a prefix): random values (distinct where 2^bits allows), distinct
    random blinding factors"""
    if bits not in _PROOFS:
        n = N_PROOFS[bits]
        rng = random.Random(0xC105E + bits)
        def distinct(bound):
            seen = {}
            while len(seen) < n:
                seen.setdefault(rng.randrange(bound), None)
            return list(seen)
        vals = distinct(1 << bits) if (1 << bits) >= 4 * n else [rng.randrange(1 << bits) for _ in range(n)]
        bfs = [x.to_bytes(32, "big") for x in distinct(bn.R)]
        _PROOFS[bits] = pp.prove_range_batch_gpu(vals, bfs, seed=0xC105E00 + bits)
    return _PROOFS[bits]


def _last_names(pp):
    """timeline names of the context's last pass; the count stays below the capacity passed"""
    from fts_gpu import _lib as L
    cap = 128
    names, ms, mads = (C.c_char_p * cap)(), (C.c_float * cap)(), (C.c_double * cap)()
    m = L.lib.fts_last_timings_ex(pp._ctx, names, ms, mads, cap)
    assert 0 < m < cap, m
    return {names[i].decode() for i in range(m)}


def _assert_path(pp, work_path):
    """the com path by the names test_gpu_knobs._golden_check uses"""
    lt = _last_names(pp)
    assert ("k_rp_com_var" in lt) == work_path and ("k_rp_fixed_all" in lt) == (not work_path), sorted(lt)


def _delta(pp, s0):
    return tuple(int(a - b) for a, b in zip(pp.pass_stats(), s0))


def _assert_clean(pp, s0, what):
    d = _delta(pp, s0)
    assert d[0] >= 1 and d[1:] == (0, 0, 0), (what, d)  # passes, failed, located, per-proof


def _honest_pass(pp, bits, B, work_path):
    proofs, coms = _honest(pp, bits)
    s0 = pp.pass_stats()
    st = pp.verify_range_proofs(proofs[:B], coms[:B])
    assert not st.any(), (B, np.flatnonzero(st)[:8])
    _assert_clean(pp, s0, (bits, B))
    _assert_path(pp, work_path)
    assert _delta(pp, s0)[0] == 1, B  # one call below the coalescing cap: one pass


@pytest.mark.parametrize("B", mp.RP32_WORK_B + mp.RP32_WORK_B_EDGE)
def test_honest_rp32_work_path(work_pp, B):
    """15 B MSM points: every layout, both sides of the transitions and of the sort switch"""
    _honest_pass(work_pp(32), 32, B, True)


@pytest.mark.parametrize("B", mp.RP32_LATENCY_B)
def test_honest_rp32_latency_path(gpu_pp, B):
    _honest_pass(gpu_pp(32), 32, B, False)


@pytest.mark.parametrize("bits,B", [(bits, B) for bits in (8, 16, 64) for B in mp.bits_B(bits)])
def test_honest_other_bit_lengths_default_path(gpu_pp, bits, B):
    """11, 13 and 17 points per proof: one proof, the last pass of k_msm_digits, the
    first of the two-level sort, 1,000 proofs"""
    _honest_pass(gpu_pp(bits), bits, B, False)


@pytest.mark.parametrize("bits", [8, 16, 64])
def test_honest_other_bit_lengths_work_path(work_pp, bits):
    _honest_pass(work_pp(bits), bits, 1000, True)


@pytest.mark.parametrize("bits", [8, 64])
def test_value_and_blinding_edges_close(gpu_pp, oracle_pp, bits):
    """values 0, 1, 2^(n-1), 2^n - 1 and blinding factors 0, 1, r - 1 in one pass with 56
    random proofs: the oracle's verdicts on the edge proofs, and a clean close"""
    pp = gpu_pp(bits)
    opp = oracle_pp.with_bit_length(bits)
    rng = random.Random(0xED6E + bits)
    vals = [0, 1, 1 << (bits - 1), (1 << bits) - 1]
    bfs = [rng.randrange(bn.R) for _ in vals]
    for bf in (0, 1, bn.R - 1):
        vals.append(rng.randrange(1, 1 << bits))
        bfs.append(bf)
    n_edge = len(vals)
    vals += [rng.randrange(1 << bits) for _ in range(56)]
    bfs += [rng.randrange(bn.R) for _ in range(56)]
    proofs, coms = pp.prove_range_batch_gpu(vals, [b.to_bytes(32, "big") for b in bfs], seed=0xED6E00 + bits)
    want = [STATUS_OF[zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q,
                                     pp.rounds, bits, zkat.RangeProof.deserialize(proofs[i]))]
            for i in range(n_edge)]
    assert want == [0] * n_edge, want
    s0 = pp.pass_stats()
    st = pp.verify_range_proofs(proofs, coms)
    assert [int(s) for s in st[:n_edge]] == want
    assert not st.any(), np.flatnonzero(st)
    _assert_clean(pp, s0, bits)


# ------------------------------------------------------------------ coalesced passes
_COAL = {}


@pytest.fixture(scope="module")
def coalesce_pp(pp_raw):
    """factory: rp16 contexts with one lane and no idle window (the held queue forms
    its pass at once), one per FTS_MAIN_GROUPS value"""
    def get(main_groups):
        if main_groups not in _COAL:
            _COAL[main_groups] = _ctx(pp_raw, 16, FTS_LANES=1, FTS_IDLE_GATHER_US=0, FTS_MAIN_GROUPS=main_groups)
        return _COAL[main_groups]
    yield get
    for pp in _COAL.values():
        pp.close()
    _COAL.clear()


def _coalesced(pp, sizes, tamper=None):
    """the caller batches of `sizes` held and verified as ONE pass -> (verdicts per
    batch, pass-counter delta); tamper = (batch, proof): L_1 of that proof moved"""
    proofs, coms = _honest(pp, 16)
    proofs = list(proofs[:sum(sizes)])
    lo = [sum(sizes[:t]) for t in range(len(sizes))]
    if tamper:
        i = lo[tamper[0]] + tamper[1]
        r = zkat.RangeProof.deserialize(proofs[i])
        r.ipa.L[1] = bn.g1_add(r.ipa.L[1], bn.GEN)
        proofs[i] = r.serialize()
    batches = [pp.stage_range_proofs(proofs[a:a + m], coms[a:a + m]) for a, m in zip(lo, sizes)]
    out = [None] * len(sizes)
    try:
        s0 = pp.pass_stats()
        pp.hold(len(sizes))
        th = [threading.Thread(target=lambda t=t: out.__setitem__(t, batches[t].verify())) for t in range(len(sizes))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        d = _delta(pp, s0)
        assert [b.merged() for b in batches] == [len(sizes)] * len(sizes)
        assert d[0] == 1, d  # one pass
    finally:
        for b in batches:
            b.close()
    return out, d, proofs, coms, lo


@pytest.mark.parametrize("main_groups", [0, 1])
@pytest.mark.parametrize("sizes", mp.COALESCED_SIZES, ids=["unequal", "equal"])
def test_honest_coalesced_pass_closes(coalesce_pp, sizes, main_groups):
    """8 honest caller batches in one pass: one combination over the pass
    (FTS_MAIN_GROUPS=0) or one per caller batch (1; with unequal batches the groups are
    padded with absent proofs and gathered through `sel`)"""
    pp = coalesce_pp(main_groups)
    out, d, _, _, _ = _coalesced(pp, list(sizes))
    for t, st in enumerate(out):
        assert not st.any(), (t, np.flatnonzero(st))
    assert d == (1, 0, 0, 0), d


@pytest.mark.parametrize("main_groups", [0, 1])
def test_one_bad_proof_in_unequal_coalesced_pass(coalesce_pp, oracle_pp, main_groups):
    """the unequal batches again, the last proof of the 33-proof batch tampered: the
    reference's verdicts, one failed combination, at most that batch's 33 proofs on the
    per-proof equations, and (one combination over the pass) a locator hit"""
    pp = coalesce_pp(main_groups)
    sizes = list(mp.COALESCED_SIZES[0])
    bad = (sizes.index(33), 32)
    out, d, proofs, coms, lo = _coalesced(pp, sizes, tamper=bad)
    opp = oracle_pp.with_bit_length(16)
    i = lo[bad[0]] + bad[1]
    err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q, pp.rounds, 16,
                         zkat.RangeProof.deserialize(proofs[i]))
    assert err is not None
    for t, st in enumerate(out):
        want = [0] * sizes[t]
        if t == bad[0]:
            want[bad[1]] = STATUS_OF[err]
        assert [int(s) for s in st] == want, t
    assert d[0] == 1 and d[1] == 1 and 1 <= d[3] <= 33, d
    if not main_groups:
        assert d[2] == 1, d


# ------------------------------------------------------------------ action calls
@pytest.fixture(scope="module")
def actions(gpu_pp):
    """40 honest 2-in / 2-out transfers and 16 honest issues of 4 tokens (rp16), proved on the device"""
    from test_gpu_prove import _bf
    pp = gpu_pp(16)
    rng = random.Random(0xAC710)
    T = b"EUR"
    tw = []
    for _ in range(40):
        iv = [rng.randrange(1 << 14) for _ in range(2)]
        ov = [rng.randrange(sum(iv) + 1)]
        ov.append(sum(iv) - ov[0])
        tw.append((T, iv, [_bf(rng) for _ in iv], ov, [_bf(rng) for _ in ov]))
    tp = pp.prove_transfers_gpu(tw, seed=0xAC7100)
    transfers = [([pp.token_commit(t, v, b) for v, b in zip(iv, ib)], [pp.token_commit(t, v, b) for v, b in zip(ov, ob)],
                  p) for (t, iv, ib, ov, ob), p in zip(tw, tp)]
    iw = [(T, [rng.randrange(1 << 16) for _ in range(4)], [_bf(rng) for _ in range(4)]) for _ in range(16)]
    ip = pp.prove_issues_gpu(iw, seed=0xAC7200)
    issues = [([pp.token_commit(t, v, b) for v, b in zip(vs, bs)], p) for (t, vs, bs), p in zip(iw, ip)]
    return transfers, issues


@pytest.mark.parametrize("which", ["mixed", "transfers", "issues"])
def test_honest_action_calls_close(gpu_pp, actions, which):
    pp = gpu_pp(16)
    transfers, issues = actions
    tr = transfers if which != "issues" else []
    iss = issues if which != "transfers" else []
    s0 = pp.pass_stats()
    st_t, _, st_i, _ = pp.verify_actions(tr, iss)
    assert len(st_t) == len(tr) and len(st_i) == len(iss)
    assert not st_t.any() and not st_i.any(), (st_t, st_i)
    _assert_clean(pp, s0, which)
