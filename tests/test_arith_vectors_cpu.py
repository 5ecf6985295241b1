"""CPU: the vectors tests/test_gpu_arith.py feeds to lib/arith_check
(tests/arith_vectors.py) are checked against integers alone, so the device test
cannot pass while never entering a branch: both sides of the Montgomery
product's conditional subtraction, the carry word of the full-width moduli,
sums at, below and above the modulus, differences with and without a borrow,
both signs of both GLV halves.  Also: `arith_check --list` (no device) equals
the catalogue the device test uses, and the Python Montgomery helpers and curve
arithmetic agree with their definitions and with the oracle."""
import os
import random
import subprocess

from conftest import ROOT

import arith_vectors as AV

EXE = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "arith_check")


def test_list_equals_catalogue():
    out = subprocess.run([EXE, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [(n, int(a), int(b)) for n, a, b in (l.split() for l in out.stdout.splitlines())]
    assert got == AV.CATALOGUE
    assert len({n for n, _, _ in got}) == len(got)


def test_contract_violations_end_the_tool_before_any_launch(tmp_path):
    """a record outside its op's documented contract makes the tool exit 2 on the host,
    before it touches a device (so this runs without one)"""
    fp, fr = AV.MODS["fp"], AV.MODS["fr"]
    M = AV.MODS["p256p"]
    G = AV.aff_words(AV.CURVES["bn"], (1, 2))
    J = AV.jac_words(AV.CURVES["bn"], (1, 2), 5)
    bad = [("fp_add", [fp, 1]), ("fp_mulg", [1, fp]), ("fr_reduce_once", [2 * fr]), ("fr_inv", [fr + 5]),
           ("p256p_cond_sub", [2 * M - AV.RR, 1]), ("p256p_cond_sub", [5, 2]), ("p256n_mul", [AV.MODS["p256n"], 1]),
           ("var_base_mul", G + [fr]), ("glv_mul", [G[0], (G[1] + 1) % fp, 5]), ("vb128j", J + [1 << 127]),
           ("vb128j", [J[0], J[1], (J[2] + 1) % fp, 3]), ("straus2_128", J + [1] + J + [1 << 128]),
           ("glv_decompose_bn", [fr]), ("glv_decompose_fbn", [AV.MODS["fbnr"]]), ("bn_f2_mul", [1, 2, 3, fp]),
           ("no_such_op", [1]), ("fp_add", [1]), ("fp_add", [1, 2, 3])]
    for op, ins in bad:
        inp = tmp_path / "in.txt"
        inp.write_text(AV.format_records([(op, ins, "raw", None)]))
        out = subprocess.run([EXE, str(inp), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (op, out.returncode, out.stderr)
        assert not (tmp_path / "out.txt").exists()


def test_records_match_catalogue_arity():
    recs = AV.field_records() + AV.glv_records() + AV.group_records()
    for op, ins, kind, want in recs:
        ni, no = AV.ARITY[op]
        assert len(ins) == ni, op
        assert all(0 <= w < AV.RR for w in ins), op
        if kind == "raw":
            assert len(want) == no, op
    # every op of these families has vectors (the scalar products and the tower are
    # counted by the device test, which builds them anyway)
    rest = {"var_base_mul", "glv_mul", "vb128j", "straus2_128"}
    need = {n for n, _, _ in AV.CATALOGUE if not n.startswith(("bn_", "fbn_f", "fbn_line"))} - rest
    assert need <= {r[0] for r in recs}, need - {r[0] for r in recs}


def test_montgomery_helpers_match_their_definitions():
    rng = random.Random(1)
    for M in AV.MODS.values():
        Ri = pow(AV.RR, -1, M)
        assert AV.RR * Ri % M == 1
        for _ in range(50):
            a, b = rng.randrange(M), rng.randrange(M)
            A, B = AV.to_mont(a, M), AV.to_mont(b, M)
            assert A == a * AV.RR % M and AV.from_mont(A, M) == a
            # the product of representatives represents the product
            assert AV.from_mont(AV.mont_mul(A, B, M), M) == a * b % M
            t = AV.mont_t(A, B, M)
            assert t < 2 * M and t % M == AV.mont_mul(A, B, M)
            # the inverse formula of the device contract: A -> A^-1 R^2 represents a^-1
            if a:
                assert AV.from_mont(pow(A, -1, M) * AV.RR * AV.RR % M, M) == pow(a, -1, M)


def test_edge_sets():
    for M in AV.MODS.values():
        E = AV.edge_set(M)
        assert all(0 <= v < M for v in E) and len(set(E)) == len(E)
        assert {(-v) % M for v in E} == set(E)
        for v in (0, 1, 2, M - 1, M - 2, (M - 1) // 2, (M + 1) // 2, AV.RR % M, (1 << 32) - 1, 1 << 224):
            assert v in E
        assert any(v & ((1 << 224) - 1) == (1 << 224) - 1 for v in E)
        assert any(v and v % (1 << 32) == 0 and v + (1 << 32) >= M for v in E)


def test_product_vectors_reach_both_sides_of_the_subtraction():
    recs = AV.field_records()
    for op, m in AV.PRODUCT_OPS:
        M = AV.MODS[m]
        ts = [AV.mont_t(ins[0], ins[1], M) for o, ins, _, _ in recs if o == op]
        assert sum(t >= M for t in ts) >= 32, op
        assert sum(t < M for t in ts) >= 32, op
        if m in AV.WIDE:
            assert sum(t >= AV.RR for t in ts) >= 32, op


def test_add_sub_vectors_reach_every_case():
    recs = AV.field_records()
    for m, M in AV.MODS.items():
        s = [ins[0] + ins[1] for o, ins, _, _ in recs if o == m + "_add"]
        assert sum(v < M for v in s) >= 8 and sum(v == M for v in s) >= 8 and sum(v > M for v in s) >= 8, m
        if m in AV.WIDE:
            assert sum(v >= AV.RR for v in s) >= 8, m
            assert sum(v == AV.RR for v in s) >= 1, m  # the sum that is 2^256 exactly
        d = [(ins[0], ins[1]) for o, ins, _, _ in recs if o == m + "_sub"]
        assert sum(a < b for a, b in d) >= 8 and sum(a == b for a, b in d) >= 8 and sum(a > b for a, b in d) >= 8, m
    for m in AV.WIDE:
        M = AV.MODS[m]
        cs = [(ins[0], ins[1]) for o, ins, _, _ in recs if o == m + "_cond_sub"]
        assert sum(c == 1 for _, c in cs) >= 32 and sum(c == 0 and x >= M for x, c in cs) >= 32, m
        assert sum(c == 0 and x < M for x, c in cs) >= 32, m
    for m in ("fp", "fr"):
        M = AV.MODS[m]
        # the zero sits at lane 17 of a wave of non-zero values
        inv = [ins[0] for o, ins, _, _ in recs if o == m + "_inv"]
        assert inv[17] == 0 and all(v for i, v in enumerate(inv[:64]) if i != 17)
    for m in AV.WIDE_MUL:
        inv = [ins[0] for o, ins, _, _ in recs if o == m + "_inv"]
        assert inv[17] == 0 and all(v for i, v in enumerate(inv[:64]) if i != 17)


def test_glv_vectors():
    """the integer Babai step on the vectors: both signs of both halves occur, the
    rounding bit is set and clear, k1 + k2 lambda = k (mod r), and the halves stay
    inside what the consuming chain can recode -- here by the lattice bound, for
    every scalar: |k1| <= (1/2 + eps)(a1 + a2), |k2| <= (1/2 + eps)(|b1| + b2)"""
    for tag, (hdr, st, r, p) in AV.GLV_SETS.items():
        c = AV.header_consts(hdr, st)
        lam = AV.glv_lambda(tag)
        assert pow(lam, 3, r) == 1 and lam != 1
        assert (c["A1"] - c["NB1"] * lam) % r == 0 and (c["A2"] + c["A1"] * lam) % r == 0
        beta = AV.from_mont(c["BETA"], p)
        assert pow(beta, 3, p) == 1 and beta != 1
        G = AV.CURVES[tag].gen
        assert AV.CURVES[tag].mul(lam, G) == (G[0] * beta % p, G[1])
        # g_i = floor(2^384 b_i / r) (b2 = a1, -b1 = NB1)
        assert c["G1"] == (c["A1"] << 384) // r and c["G2"] == (c["NB1"] << 384) // r
        assert (c["A1"] + c["A2"]) // 2 + 2 < AV.GLV_BOUND[tag] and (c["NB1"] + c["A1"]) // 2 + 2 < AV.GLV_BOUND[tag]
        # the bound the header comment states (glv.hpp: 2^126, fp256bn.hpp: 2^128) is not tighter than what holds
        stated = {"bn": 1 << 126, "fbn": 1 << 128}[tag]
        assert (c["A1"] + c["A2"]) // 2 + 2 < stated and (c["NB1"] + c["A1"]) // 2 + 2 < stated
        ks = AV.glv_scalars(tag)
        s1 = s2 = cy1 = cy0 = 0
        for k in ks:
            k1, k2 = AV.glv_decompose(k, c)
            assert (k1 + k2 * lam - k) % r == 0
            assert abs(k1) < AV.GLV_BOUND[tag] and abs(k2) < AV.GLV_BOUND[tag]
            s1 += k1 < 0
            s2 += k2 < 0
            bit = ((k * c["G1"]) >> 383) & 1
            cy1 += bit
            cy0 += 1 - bit
        assert s1 >= 1 and s2 >= 1 and len(ks) - s1 >= 1 and len(ks) - s2 >= 1
        assert cy1 >= 32 and cy0 >= 32
    want = [("glv_decompose_" + t, len(AV.glv_scalars(t))) for t in AV.GLV_SETS]
    got = AV.glv_records()
    assert [(op, sum(1 for r_ in got if r_[0] == op)) for op, _ in want] == want


def test_list_glv_names_the_op():
    out = subprocess.run([EXE, "--list-glv"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert [(n, int(a), int(b)) for n, a, b in (l.split() for l in out.stdout.splitlines())] == AV.GLV_CATALOGUE


def test_fbn_glv_mul_scalars_have_the_properties_noted():
    """FBN_GLV_KS: each scalar decomposes as its note says, on-curve operands, and no k can
    carry into window 32 (the lattice bound keeps nibble 31 of both halves at 7 or less)"""
    hdr, st, r, p = AV.GLV_SETS["fbn"]
    c = AV.header_consts(hdr, st)
    assert (c["A1"] + c["A2"]) // 2 + 2 < 1 << 127 and (c["NB1"] + c["A1"]) // 2 + 2 < 1 << 127
    ks = AV.fbn_glv_scalars()
    dec = [AV.glv_decompose(k, c) for k in ks]
    assert dec[:6] == [(0, 0), (1, 0), (2, 0), (-1, 0), (0, 1), (-1, 1)]
    k1, k2 = dec[6]
    assert abs(k1) >> 108 == 0x7ffff and k1 < 0 < k2
    assert dec[7] == (0x7fffffffffff00000000000000000000, 0) and dec[8] == (5 << 100, 0)
    assert all(abs(a) < 1 << 127 and abs(b) < 1 << 127 for a, b in dec)
    recs = AV.fbn_glv_records()
    assert len(recs) == 2 * len(ks) and len(ks) == len(AV.FBN_GLV_KS) + 8
    C = AV.CURVES["fbn"]
    for op, ins, kind, want in recs:
        assert op == "fbn_glv_mul" and kind == "jac:fbn" and ins[2] < r
        P = (AV.from_mont(ins[0], p), AV.from_mont(ins[1], p))
        assert C.on(P) and want == (C.mul(ins[2], P) if ins[2] else None)


def test_curve_arithmetic_agrees_with_the_oracle():
    from oracle import bn254 as bn, ecdsa_p256 as P2, idemix as OI
    rng = random.Random(2)
    for _ in range(4):
        k, j = rng.randrange(bn.R), rng.randrange(bn.R)
        C = AV.CURVES["bn"]
        P, Q = C.mul(k, C.gen), C.mul(j, C.gen)
        assert P == bn.g1_mul(bn.GEN, k) and C.add(P, Q) == bn.g1_add(P, Q) and C.add(P, P) == bn.g1_add(P, P)
        C = AV.CURVES["p256"]
        assert C.mul(k % P2.N, C.gen) == P2.mul(k % P2.N, P2.G)
        C = AV.CURVES["fbn"]
        F = OI.FP256BNC
        assert C.mul(k, C.gen) == F.mul((1, 2), k) and C.on(C.mul(k, C.gen))
    # the forms the device takes normalise back to the point, whatever the denominator
    for cn, C in AV.CURVES.items():
        P = C.mul(12345, C.gen)
        for z in (1, C.p - 1, 0x1234567):
            assert AV.norm_jac(C, AV.jac_words(C, P, z)) == P
        assert AV.norm_jac(C, AV.jac_words(C, None, 0, (5, 6))) is None
    C = AV.CURVES["bn"]
    assert AV.norm_xyzz(C, AV.xyzz_words(C, C.gen, C.p - 1)) == C.gen


def test_group_vectors_cover_the_exceptional_cases():
    """every addition formula gets P + P under different denominators, P + (-P),
    P + 2P and the identity on each side its contract admits"""
    recs = AV.group_records()
    adds = ["g1j_add_affine", "g1j_add", "madd_inl", "add_inl", "xmadd_inl", "xadd_inl", "p256_pj_add",
            "p256_pj_madd", "fbn_pj_add", "fbn_pj_madd"]
    for op in adds:
        mine = [r for r in recs if r[0] == op]
        assert sum(r[3] is None for r in mine) >= 3, op  # P + (-P) (and identity + identity)
        assert len(mine) >= 30, op
    for op, ins, kind, want in recs:
        if kind.startswith("jac:") and want is not None:
            assert AV.CURVES[kind[4:]].on(want), op
