"""CPU: the vectors tests/test_gpu_com_chain.py feeds to lib/arith_check
(tests/com_chain_vectors.py) are consistent with the oracle's integers on their
own -- every expectation is sum k_i P_i by oracle/bn254.py, recomputed here term
by term with phi applied as a map on coordinates -- and every edge case the
device code has a branch for is present.  `arith_check --list-chain` (no device)
names the op with the arity the vectors use."""
import os
import subprocess

from conftest import ROOT

from oracle import bn254 as bn

import arith_vectors as AV
import com_chain_vectors as CV

EXE = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "arith_check")
BETA = AV.from_mont(AV.header_consts("glv.hpp", "Glv")["BETA"], bn.P)


def _phi(P):
    return None if P is None else (P[0] * BETA % bn.P, P[1])


def _aff(w):
    return None if w == [0, 0] else (AV.from_mont(w[0], bn.P), AV.from_mont(w[1], bn.P))


def test_list_chain_names_the_op():
    out = subprocess.run([EXE, "--list-chain"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {n: (int(a), int(b)) for n, a, b in (l.split() for l in out.stdout.splitlines())}
    assert got == CV.ARITY
    # the primitives' catalogue is listed apart and unchanged
    out = subprocess.run([EXE, "--list"], capture_output=True, text=True, timeout=60)
    assert not set(CV.ARITY) & {l.split()[0] for l in out.stdout.splitlines()}


def test_contract_violations_end_the_tool_before_any_launch(tmp_path):
    G = AV.aff_words(AV.CURVES["bn"], (1, 2))
    J = AV.jac_words(AV.CURVES["bn"], (1, 2), 5)
    off = [G[0], (G[1] + 1) % bn.P]
    halves = [1, 0, 1, 0, 1, 0, 1, 0]
    bad = [("straus4_ctab", off + J + halves), ("straus4_ctab", [bn.P, 0] + J + halves),
           ("straus4_ctab", G + [J[0], J[1], (J[2] + 1) % bn.P] + halves),
           ("straus4_ctab", G + J + [1 << 127, 0, 1, 0, 1, 0, 1, 0]), ("straus4_ctab", G + J + [1, 2, 1, 0, 1, 0, 1, 0]),
           ("straus4_ctab", G + J + halves[:-1])]
    for op, ins in bad:
        inp = tmp_path / "in.txt"
        inp.write_text(AV.format_records([(op, ins, "raw", None)]))
        out = subprocess.run([EXE, str(inp), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (op, out.returncode, out.stderr)
        assert not (tmp_path / "out.txt").exists()


def test_phi_is_multiplication_by_lambda():
    assert pow(CV.LAM, 3, bn.R) == 1 and CV.LAM != 1 and pow(BETA, 3, bn.P) == 1 and BETA != 1
    P = bn.g1_mul(bn.GEN, 0xC0FFEE)
    assert bn.g1_mul(P, CV.LAM) == _phi(P)


def test_straus_vectors_are_self_consistent_and_cover_the_branches():
    recs = CV.straus_records()
    by = {}
    for op, ins, kind, want, tag in recs:
        assert op == "straus4_ctab" and kind == "jac:bn" and len(ins) == CV.ARITY[op][0]
        D, S = _aff(ins[:2]), AV.norm_jac(AV.CURVES["bn"], ins[2:5])
        assert bn.on_curve(D) and bn.on_curve(S) and bn.on_curve(want)
        a1, s1, a2, s2, b1, t1, b2, t2 = ins[5:]
        assert all(m < (1 << 127) for m in (a1, a2, b1, b2)) and all(s in (0, 1) for s in (s1, s2, t1, t2))
        # sum k_i P_i term by term, phi as the map (x, y) -> (beta x, y)
        terms = [(a1, s1, D), (a2, s2, _phi(D)), (b1, t1, S), (b2, t2, _phi(S))]
        acc = None
        for m, s, Pt in terms:
            t = bn.g1_mul(Pt, m)
            acc = bn.g1_add(acc, bn.g1_neg(t) if s else t)
        assert acc == want, tag
        by.setdefault(tag, []).append((D, S, (a1, s1, a2, s2, b1, t1, b2, t2), want))
    # every magnitude in every position, and in all four at once
    for pos in range(4):
        for m in CV.MAGS:
            (_, _, h, _), = by["mag_%d_%x" % (pos, m)]
            assert h[2 * pos] == m
    for m in CV.MAGS:
        (_, _, h, _), = by["mag_all_%x" % m]
        assert h[0] == h[2] == h[4] == h[6] == m
    # all sixteen sign combinations, twice (random and edge magnitudes)
    for sg in range(16):
        got = by["signs_%x" % sg]
        assert len(got) == 2 and all((h[1], h[3], h[5], h[7]) == tuple((sg >> q) & 1 for q in range(4)) for _, _, h, _ in got)
    assert all(D == S for D, S, _, _ in by["d_eq_s"]) and len(by["d_eq_s"]) >= 4
    assert all(D == bn.g1_neg(S) for D, S, _, _ in by["d_eq_neg_s"]) and len(by["d_eq_neg_s"]) >= 4
    # 1 D + 1 S: the accumulator holds D when S's first row (= +-D) arrives
    assert any(h == (1, 0, 0, 0, 1, 0, 0, 0) and w == bn.g1_mul(D, 2) for D, _, h, w in by["d_eq_s"])
    assert any(h == (1, 0, 0, 0, 1, 0, 0, 0) and w is None for _, _, h, w in by["d_eq_neg_s"])
    assert all(S == _phi(D) for D, S, _, _ in by["s_eq_phi_d"]) and len(by["s_eq_phi_d"]) >= 6
    assert any(h == (0, 0, 1, 0, 1, 0, 0, 0) and w == bn.g1_mul(S, 2) for _, S, h, w in by["s_eq_phi_d"])
    assert any(h == (0, 0, 1, 0, 1, 1, 0, 0) and w is None for _, _, h, w in by["s_eq_phi_d"])
    assert all(D is None and S is not None for D, S, _, _ in by["id_d"]) and len(by["id_d"]) >= 2
    assert all(D is not None and S is None for D, S, _, _ in by["id_s"]) and len(by["id_s"]) >= 2
    assert all(D is None and S is None and w is None for D, S, _, w in by["id_both"]) and len(by["id_both"]) >= 2
    # S reaches the device with a denominator other than 1
    assert all(ins[4] != AV.to_mont(1, bn.P) for _, ins, _, _, _ in recs)
