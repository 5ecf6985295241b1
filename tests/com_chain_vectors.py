"""Vectors for the com chain's device function, as lib/arith_check runs it (op
`straus4_ctab`, listed by `arith_check --list-chain`):

  straus4_ctab(...)    a1 (s1 D) + a2 phi(s2 D) + b1 (t1 S) + b2 phi(t2 S) over the
                       proof's affine table (glv.hpp), k_rp_com_var's chain; the tool
                       builds the table with ctab_build8 as k_rp_com_tab does

There are no vectors for an affine + affine first addition (`xadd_aff2`) here on
purpose: that part of the change is not in the library ("Affine +
affine first addition"), and its op and vectors went with it.

Every expectation is a point computed with oracle/bn254.py's integer arithmetic
(g1_add, g1_mul); phi is multiplication by the lambda that
device/glv.hpp's constants define (arith_vectors.glv_lambda).  Records have the
shape of arith_vectors': (op, operand words, result kind, expected point).
tests/test_com_chain_vectors_cpu.py checks the vectors against themselves and
that every named edge case is present; tests/test_gpu_com_chain.py runs them."""
import random

from oracle import bn254 as bn

import arith_vectors as AV

C = AV.CURVES["bn"]
ARITY = {"straus4_ctab": (13, 3)}
LAM = AV.glv_lambda("bn")
# magnitudes at the recoding's digit boundaries (7, 8, 9: carry
# out of a window at 9; 15, 16: the next window), a word boundary, the top window
MAGS = [0, 1, 7, 8, 9, 15, 16, 1 << 64, 1 << 126, (1 << 127) - 1]


def _pt(rng):
    return bn.g1_mul(bn.GEN, rng.randrange(1, bn.R))


def straus_value(D, S, halves):
    """the group element the chain must return: halves = ((a1, s1), (a2, s2), (b1, t1), (b2, t2))"""
    (a1, s1), (a2, s2), (b1, t1), (b2, t2) = halves
    kd = ((-a1 if s1 else a1) + (-a2 if s2 else a2) * LAM) % bn.R
    ks = ((-b1 if t1 else b1) + (-b2 if t2 else b2) * LAM) % bn.R
    return bn.g1_add(bn.g1_mul(D, kd), bn.g1_mul(S, ks))


def straus_cases():
    """(tag, D, S, zS, halves): D affine, S given to the device as Jacobian with
    denominator zS (S None: z = 0)"""
    rng = random.Random(0x57A4)
    cases = []

    def mag():
        return rng.randrange(1 << 127)

    def signs():
        return [rng.randrange(2) for _ in range(4)]

    def z():
        return rng.randrange(2, bn.P)

    # every magnitude in every position, the other three random
    for pos in range(4):
        for m in MAGS:
            ms = [mag() for _ in range(4)]
            ms[pos] = m
            cases.append(("mag_%d_%x" % (pos, m), _pt(rng), _pt(rng), z(), list(zip(ms, signs()))))
    # all sixteen sign combinations, on one random set and on a set of edge magnitudes
    D, S, zs = _pt(rng), _pt(rng), z()
    for ms in ([mag() for _ in range(4)], [9, 1 << 126, 15, (1 << 127) - 1]):
        for sg in range(16):
            cases.append(("signs_%x" % sg, D, S, zs, list(zip(ms, [(sg >> q) & 1 for q in range(4)]))))
    # all four magnitudes at an edge at once
    for m in MAGS:
        cases.append(("mag_all_%x" % m, _pt(rng), _pt(rng), z(), [(m, s) for s in signs()]))
    # D = S and D = -S: the accumulator meets the other point's row (1 D then 1 S:
    # doubling resp. the identity), then random scalars
    for tag, f in (("d_eq_s", lambda p: p), ("d_eq_neg_s", bn.g1_neg)):
        D = _pt(rng)
        cases.append((tag, D, f(D), z(), [(1, 0), (0, 0), (1, 0), (0, 0)]))
        cases.append((tag, D, f(D), z(), [(17, 0), (0, 0), (17, 0), (0, 0)]))
        for _ in range(3):
            cases.append((tag, D, f(D), z(), list(zip([mag() for _ in range(4)], signs()))))
    # S = phi(D): D's beta*x rows are S's x rows, so the accumulator meets its own table
    # entry (a2 phi(D) then b1 S with a2 = b1: the doubling branch; opposite signs: identity)
    D = _pt(rng)
    S = bn.g1_mul(D, LAM)
    for halves in ([(0, 0), (1, 0), (1, 0), (0, 0)], [(0, 0), (1, 0), (1, 1), (0, 0)],
                   [(0, 0), (0x123, 1), (0x123, 1), (0, 0)], [(5, 0), (8, 1), (8, 1), (3, 1)]):
        cases.append(("s_eq_phi_d", D, S, z(), halves))
    for _ in range(3):
        cases.append(("s_eq_phi_d", D, S, z(), list(zip([mag() for _ in range(4)], signs()))))
    # identities: D, S, both
    for tag, hd, hs in (("id_d", False, True), ("id_s", True, False), ("id_both", False, False)):
        for _ in range(2):
            cases.append((tag, _pt(rng) if hd else None, _pt(rng) if hs else None, z(),
                          list(zip([mag() for _ in range(4)], signs()))))
    return cases


def straus_records():
    recs = []
    for tag, D, S, zs, halves in straus_cases():
        ins = AV.aff_words(C, D) + AV.jac_words(C, S, zs)
        for m, s in halves:
            ins += [m, s]
        recs.append(("straus4_ctab", ins, "jac:bn", straus_value(D, S, halves), tag))
    return recs


_CACHE = {}


def all_records():
    """computed once per process (the expectations are a few hundred oracle products)"""
    if "all" not in _CACHE:
        _CACHE["all"] = straus_records()
    return _CACHE["all"]


def format_records(recs):
    return AV.format_records([r[:4] for r in recs])
