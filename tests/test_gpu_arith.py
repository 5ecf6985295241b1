"""GPU: the device arithmetic primitives against integer oracles, operand by
operand (lib/arith_check, csrc/tools/arith_check.cpp): the BN254 Fp / Fr products
in inline assembly and the constant-time GCD inverse (device/field.hpp), the
full-width Montgomery code of P-256 and FP256BN (device/p256.hpp), the Jacobian
and XYZZ group laws with their exceptional branches (device/g1.hpp,
device/fixed_base.hpp), GLV decomposition and the 128-bit chains
(device/glv.hpp), and the Fp2 / Fp6 / Fp12 tower of both pairing curves
(device/pairing.hpp).  The vectors (tests/arith_vectors.py) sit on the operands
where multi-limb code goes wrong; tests/test_arith_vectors_cpu.py checks that
they reach the branches.  Every expectation is integer arithmetic; comparison is
exact equality of canonical values.  The tool runs once per session."""
import os
import subprocess
import time

import pytest

from conftest import ROOT

import arith_vectors as AV

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "arith_check")
# ten times the tool's wall time on its first MI355X run (MEASURED_S), at least 60 s
MEASURED_S = 0.40  # 47,862 records, process start to exit, device initialisation included
TIMEOUT_S = max(60.0, 10 * MEASURED_S)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """all vectors through one invocation of the tool: {op: [(record, result words)]}"""
    assert os.path.exists(EXE), "lib/arith_check is not built"
    recs = AV.all_records()
    d = tmp_path_factory.mktemp("arith")
    inp, outp = d / "in.txt", d / "out.txt"
    inp.write_text(AV.format_records(recs))
    t0 = time.time()
    out = subprocess.run([EXE, str(inp), str(outp)], capture_output=True, text=True, timeout=TIMEOUT_S)
    wall = time.time() - t0
    assert out.returncode == 0, out.stdout + out.stderr
    res = AV.parse_results(outp.read_text())
    assert len(res) == len(recs)
    by = {}
    for r, w in zip(recs, res):
        assert len(w) == AV.ARITY[r[0]][1], r[0]
        by.setdefault(r[0], []).append((r, w))
    fam = {"field": AV.field_records(), "glv": AV.glv_records(), "group": AV.group_records(),
           "scalar": AV.scalar_records(), "tower": AV.tower_records()}
    print("arith_check: %d records in %.2f s (%s)" % (len(recs), wall,
                                                      ", ".join("%s %d" % (k, len(v)) for k, v in fam.items())))
    return by


def _check(run, ops):
    bad = []
    n = 0
    for op in ops:
        assert run.get(op), "no vectors for " + op
        for lane, ((_, ins, kind, want), words) in enumerate(run[op]):
            n += 1
            try:
                got = AV.normalise(kind, words)
            except AssertionError as e:
                got = "not normalisable: %s" % e
            if got != want:
                bad.append("%s lane %d: in %s\n  got  %s\n  want %s" % (
                    op, lane, " ".join("%x" % w for w in ins), got, want))
    assert not bad, "%d of %d records differ\n%s" % (len(bad), n, "\n".join(bad[:8]))


def test_every_catalogue_op_has_vectors(run):
    assert set(run) == {n for n, _, _ in AV.CATALOGUE}


@pytest.mark.parametrize("m", list(AV.MODS))
def test_field_ops(run, m):
    """add, sub, neg/dbl, the products, to/from Montgomery, the inverse (zero at lane 17)
    and the reduction helpers of one modulus"""
    _check(run, [n for n, _, _ in AV.CATALOGUE if n.startswith(m + "_")])


def test_lt256(run):
    _check(run, ["lt256"])


@pytest.mark.parametrize("op", ["g1j_add_affine", "g1j_add", "madd_inl", "add_inl", "xmadd_inl", "xadd_inl"])
def test_bn254_additions(run, op):
    """generic pairs, P + P under different denominators, P + (-P), P + 2P and the
    identity (also encoded with non-zero x, y) on each side the contract admits"""
    _check(run, [op])


def test_bn254_doublings_and_conversions(run):
    _check(run, ["g1j_dbl", "g1x_dbl", "g1j_to_affine", "g1x_to_jac", "g1j_eq"])


@pytest.mark.parametrize("c", ["p256", "fbn"])
def test_full_width_curve_points(run, c):
    _check(run, [c + "_pj_dbl", c + "_pj_add", c + "_pj_madd", c + "_on_curve"])


@pytest.mark.parametrize("op", ["var_base_mul", "glv_mul", "vb128j", "straus2_128"])
def test_scalar_products(run, op):
    _check(run, [op])


def test_fbn_glv_mul(tmp_path):
    """fbn::glv_mul_tab (device/fbn_glv.hpp), the FP256BN nym kernels' variable-base product,
    against the oracle's k * Q: the scalars of AV.FBN_GLV_KS and eight random ones on two
    points.  Its op is listed apart from the catalogue (--list-glv), so it has a run of its own"""
    recs = AV.fbn_glv_records()
    inp, outp = tmp_path / "in.txt", tmp_path / "out.txt"
    inp.write_text(AV.format_records(recs))
    out = subprocess.run([EXE, str(inp), str(outp)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert out.returncode == 0, out.stdout + out.stderr
    res = AV.parse_results(outp.read_text())
    assert len(res) == len(recs) and all(len(w) == 3 for w in res)
    _check({"fbn_glv_mul": list(zip(recs, res))}, ["fbn_glv_mul"])


@pytest.mark.parametrize("tag", ["bn", "fbn"])
def test_glv_decompose(run, tag):
    """the device Babai step equals the integer one limb for limb; with the returned
    signs k1 + k2 lambda = k (mod r), and both halves fit the consuming chain"""
    op = "glv_decompose_" + tag
    _check(run, [op])
    r, lam = AV.GLV_SETS[tag][2], AV.glv_lambda(tag)
    for (_, (k,), _, _), (k1, s1, k2, s2) in run[op]:
        assert s1 in (0, 1) and s2 in (0, 1)
        assert ((-k1 if s1 else k1) + (-k2 if s2 else k2) * lam - k) % r == 0
        assert k1 < AV.GLV_BOUND[tag] and k2 < AV.GLV_BOUND[tag]


@pytest.mark.parametrize("tag", ["bn", "fbn"])
@pytest.mark.parametrize("level", ["f2", "f6", "f12", "line"])
def test_tower(run, tag, level):
    """Fp2 / Fp6 / Fp12 of one curve against the dense integer tower: cyc_sqr on
    cyclotomic inputs equals the generic square, frob<n> equals a^(p^n), line_mul
    equals the dense product with the line embedded by the twist type"""
    _check(run, [n for n, _, _ in AV.CATALOGUE if n.startswith("%s_%s_" % (tag, level))])
