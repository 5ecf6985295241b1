"""GPU: the add-only accumulators in extended Jacobian (XYZZ) coordinates
(device/g1.hpp G1X, fixed_base.hpp xmadd_inl / fb_sum_w, msm.hip k_msm_chunks).

Every expectation is the oracle's (oracle/bn254.py group law, oracle/zkat.py
commitments, the C oracle's verdicts), never another device path.  The cases aim
at what the new formulas treat apart from the straight line: an accumulator that
meets its own point again (doubling), its negative (identity, then more points),
the identity as an input, a single non-zero digit (copy only), no non-zero digit.

The wide (20/22-bit) tables see only hash outputs in the byte-for-byte H' / com tests
of test_gpu_rp.py and test_gpu_coalesce.py; test_gpu_fixed_base.py sends chosen
scalars through them (a proof's Delta), checks every width's recoding and products
at the digit edges and reads the built tables back entry by entry."""
import random

import pytest

from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

RNG = random.Random(0x58595A5A)
P = bn.g1_mul(bn.GEN, RNG.randrange(1, bn.R))
Q = bn.g1_mul(bn.GEN, RNG.randrange(1, bn.R))
K = RNG.randrange(1, bn.R)


def _pts(points):
    return b"".join(bn.g1_bytes(p) for p in points)


def _scs(scalars):
    return b"".join(k.to_bytes(32, "big") for k in scalars)


def _run(pp, points, scalars):
    st = pp.stage_msm(_pts(points), _scs(scalars))
    try:
        return bytes(st.run())
    finally:
        st.close()


@pytest.mark.parametrize("m", [2, 3, 9])
def test_msm_doubling_inside_a_chunk(gpu_pp, m):
    """m copies of P under one scalar share every bucket: the chunk accumulator meets
    its own point (P = 0, R = 0 -> doubling), then adds on; at m = 9 a bucket holds a
    chunk of 8 and a chunk of 1, joined by k_msm_bucket_sum"""
    got = _run(gpu_pp(64), [P] * m, [K] * m)
    assert got == bn.g1_bytes(bn.g1_mul(P, m * K % bn.R))


def test_msm_cancellation_inside_a_chunk(gpu_pp):
    """P then -P in one bucket (P = 0, R != 0 -> identity), then more points or none;
    the identity as the first input point"""
    pp = gpu_pp(64)
    nP = bn.g1_neg(P)
    assert _run(pp, [P, nP, Q], [K, K, K]) == bn.g1_bytes(bn.g1_mul(Q, K))
    assert _run(pp, [P, nP, P, nP], [K] * 4) == bytes(64)
    assert _run(pp, [None, P, P], [K] * 3) == bn.g1_bytes(bn.g1_mul(P, 2 * K % bn.R))


@pytest.mark.parametrize("n", [2, 9, 17, 64])
def test_msm_random_with_special_scalars(gpu_pp, n):
    rng = random.Random(0x58000 + n)
    points = [bn.g1_mul(bn.GEN, rng.randrange(1, bn.R)) for _ in range(n)]
    scalars = [rng.randrange(bn.R) for _ in range(n)]
    special = [0, 1, bn.R - 1, 1 << 126]
    if n < len(special):
        special = special[2:]  # n = 2: r - 1 and 2^126 (0 and 1 ride along at n >= 9)
    for i, s in enumerate(special):
        scalars[i * (n // len(special))] = s
    got = _run(gpu_pp(64), points, scalars)
    assert got == bn.g1_bytes(bn.g1_msm(points, scalars))


def test_grouped_plan_verdicts(gpu_pp, oracle_pp):
    """64 8-bit proofs, 2 tampered: the batch check fails, the group test and its
    grouped MSM (sel indirection, G > 1) run over k_msm_chunks; verdicts = the oracle's"""
    from oracle import cref, zkat
    pp = gpu_pp(8)
    opp = oracle_pp.with_bit_length(8)
    n = 64
    proofs, coms = pp.prove_range_batch([(37 * i + 5) % 256 for i in range(n)],
                                        [(0x58 + i).to_bytes(32, "big") for i in range(n)], seed=0x58)
    t = zkat.RangeProof.deserialize(proofs[9])
    t.ipa.L[1] = bn.g1_add(t.ipa.L[1], bn.GEN)
    proofs[9] = t.serialize()
    t = zkat.RangeProof.deserialize(proofs[50])
    t.data.T2 = bn.g1_neg(t.data.T2)
    proofs[50] = t.serialize()
    want = cref.rp_verify_many(opp, coms, proofs, threads=1)
    assert [i for i, s in enumerate(want) if s != 0] == [9, 50], want
    st = [int(s) for s in pp.verify_range_proofs(proofs, coms)]
    names = sorted(pp.last_timings())
    print("kernels:", names)
    assert st == want
    assert "fb:k_rlc_group_final" in names and "fb:k_msm_chunks" in names, names  # the group test ran


# digits of the signed 16-bit recoding: zero digits, the carry into the next window
# (2^15 + 1 .. 2^16 - 1), a single non-zero digit (copy only), the all-zero scalar
FB_SCALARS = [0, 1, 1 << 15, (1 << 15) + 1, (1 << 16) - 1, 1 << 16, bn.R - 1, bn.R - (1 << 16), 0x5A5A << 112]


def test_fixed_base_16bit_tables(gpu_pp, oracle_pp):
    """type ped0 + value ped1 + bf ped2 for every (value, bf) of FB_SCALARS^2 against the
    oracle's commitment: token_commit (the library's commitment; its value is a u64, so
    the values below 2^64) and, for all 81 pairs, the device's re-commitment over the
    16-bit tables (fts_token_open_batch: fb_mul_acc per generator), which accepts the
    oracle's commitment and rejects the commitment of another pair"""
    import fts_gpu as F
    from oracle import zkat
    pp = gpu_pp(64)
    T = b"XYZZ"
    pairs = [(v, bf) for v in FB_SCALARS for bf in FB_SCALARS]
    coms = [bn.g1_bytes(zkat.token_commit(oracle_pp.ped, T, v, bf)) for v, bf in pairs]
    for (v, bf), com in zip(pairs, coms):
        if v < 1 << 64:
            assert pp.token_commit(T, v, bf.to_bytes(32, "big")) == com, (v, bf)
    ops = [(com, T, v.to_bytes(32, "big"), bf.to_bytes(32, "big")) for (v, bf), com in zip(pairs, coms)]
    assert [int(s) for s in pp.check_openings(ops)] == [F.FTS_OK] * len(ops)
    # every commitment against the next pair's opening (all 81 commitments are distinct)
    assert len(set(coms)) == len(coms)
    shifted = [(coms[(i + 1) % len(ops)],) + ops[i][1:] for i in range(len(ops))]
    assert [int(s) for s in pp.check_openings(shifted)] == [F.FTS_E_OPEN_MISMATCH] * len(ops)
