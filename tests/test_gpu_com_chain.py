"""GPU: the work path's com chain with one lane per proof (k_rp_com_tab builds the
proof's affine table, k_rp_com_var runs ONE joint GLV/Straus chain over it).

1. tests/com_chain_vectors.py through lib/arith_check (op straus4_ctab), one
   invocation, against oracle/bn254.py integers.
2. Work-path passes (FTS_COM_FIXED_MAX=0) of 1, 63, 64, 65 and 130 honest proofs
   at 8 bits -- the sizes around the 64-lane wave / block of one lane per proof --
   each with a malformed proof (its lane exits), a proof with D replaced by -D and
   one with D replaced by C (the table of D then holds the point the chain adds
   last).  Every verdict equals the C oracle's; com, every H'_i and x0 equal
   zkat.rp_verify's trace for a sample of the honest proofs (the Python oracle is
   slow), and com of the two altered proofs -- which the oracle rejects at its
   first equation, before it traces com -- equals the same lines of the oracle
   (rp_verify's com, restated below from its traced challenges and checked
   against its own trace on an honest proof).  One pass of 65 proofs at 64 bits."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

from oracle import bn254 as bn, cref, zkat

import arith_vectors as AV
import com_chain_vectors as CV

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "arith_check")
TIMEOUT_S = 60.0  # as tests/test_gpu_arith.py: the tool takes well under a second


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """all vectors through one invocation of the tool: {op: [(record, result words)]}"""
    assert os.path.exists(EXE), "lib/arith_check is not built"
    recs = CV.all_records()
    d = tmp_path_factory.mktemp("com_chain")
    inp, outp = d / "in.txt", d / "out.txt"
    inp.write_text(CV.format_records(recs))
    out = subprocess.run([EXE, str(inp), str(outp)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert out.returncode == 0, out.stdout + out.stderr
    res = AV.parse_results(outp.read_text())
    assert len(res) == len(recs)
    by = {}
    for r, w in zip(recs, res):
        assert len(w) == CV.ARITY[r[0]][1], r[0]
        by.setdefault(r[0], []).append((r, w))
    return by


@pytest.mark.parametrize("op", ["straus4_ctab"])
def test_vectors(run, op):
    bad = []
    assert run.get(op), "no vectors for " + op
    for lane, ((_, ins, kind, want, tag), words) in enumerate(run[op]):
        try:
            got = AV.normalise(kind, words)
        except AssertionError as e:
            got = "not normalisable: %s" % e
        if got != want:
            bad.append("%s lane %d (%s): in %s\n  got  %s\n  want %s" % (
                op, lane, tag, " ".join("%x" % w for w in ins), got, want))
    assert not bad, "%d of %d records differ\n%s" % (len(bad), len(run[op]), "\n".join(bad[:8]))


# ------------------------------------------------------------------ whole passes
_WORK_CTX = {}


def _work_path_pp(pp_raw, bits):
    """a context whose passes all take the work path for com (FTS_COM_FIXED_MAX=0), one
    dispatcher lane (as tests/test_gpu_rp.py's)"""
    import fts_gpu
    if bits not in _WORK_CTX:
        old = {k: os.environ.get(k) for k in ("FTS_COM_FIXED_MAX", "FTS_LANES")}
        os.environ.update(FTS_COM_FIXED_MAX="0", FTS_LANES="1")
        try:
            _WORK_CTX[bits] = fts_gpu.PublicParams(pp_raw, bit_length=bits, device=0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _WORK_CTX[bits]


def _intermediates(pp, i):
    from fts_gpu import _lib as L
    k, n = pp.rounds, pp.bit_length
    ch = C.create_string_buffer(32 * (8 + 2 * k))
    com = C.create_string_buffer(64)
    hp = C.create_string_buffer(64 * n)
    L.check("dbg", L.lib.fts_debug_rp_intermediates(pp._ctx, i, ch, com, hp))
    vals = [int.from_bytes(ch.raw[32 * q:32 * q + 32], "big") for q in range(8 + 2 * k)]
    return vals, com.raw, [hp.raw[64 * q:64 * q + 64] for q in range(n)]


def _oracle_com(opp, rp, tr):
    """rp_verify's com and H' (oracle/zkat.py, verifyIPA's first part) from the challenges
    it traced: for proofs it rejects at its first equation, before it reaches these lines"""
    d, x, y, z = rp.data, tr["x"], tr["y"], tr["z"]
    z2 = z * z % bn.R
    c = bn.g1_add(bn.g1_mul(d.D, x), d.C)
    hp = []
    yp = 1
    for i in range(len(opp.left)):
        c = bn.g1_sub(c, bn.g1_mul(opp.left[i], z))
        hp.append(bn.g1_mul(opp.right[i], pow(yp, bn.R - 2, bn.R)))
        c = bn.g1_add(c, bn.g1_mul(hp[i], (z * yp + z2 * pow(2, i, bn.R)) % bn.R))
        yp = yp * y % bn.R
    return bn.g1_sub(c, bn.g1_mul(opp.P, d.Delta)), hp


def _run_pass(pp, opp, bits, nhonest, traced, seed):
    """nhonest honest proofs, then D -> -D, D -> C, and a malformed proof in the middle;
    traced: the pass positions whose com, H' and x0 the Python oracle traces (honest ones)"""
    rounds = bits.bit_length() - 1
    vals = [(i * 0x9E3779B97F4A7C15 + seed) & ((1 << bits) - 1) for i in range(nhonest + 2)]
    bfs = [((i + 1) * 0x1234567 + seed).to_bytes(32, "big") for i in range(nhonest + 2)]
    proofs, coms = pp.prove_range_batch(vals, bfs, seed=seed)
    proofs, coms = list(proofs), list(coms)
    i_neg, i_c = nhonest, nhonest + 1
    r = zkat.RangeProof.deserialize(proofs[i_neg])
    r.data.D = bn.g1_neg(r.data.D)
    proofs[i_neg] = r.serialize()
    r = zkat.RangeProof.deserialize(proofs[i_c])
    r.data.D = r.data.C
    proofs[i_c] = r.serialize()
    i_bad = nhonest // 2  # the malformed proof sits inside a wave of running lanes
    proofs.insert(i_bad, proofs[0][:-1])
    coms.insert(i_bad, coms[0])
    shift = lambda i: i + (i >= i_bad)
    i_neg, i_c = shift(i_neg), shift(i_c)
    st = [int(s) for s in pp.verify_range_proofs(proofs, coms)]
    want = cref.rp_verify_many(opp, coms, proofs, threads=1)
    assert st == want, (st, want)
    assert st[i_bad] == 1 and st[i_neg] != 0 and st[i_c] != 0 and sum(s != 0 for s in st) == 3
    lt = pp.last_timings()
    assert "k_rp_com_var" in lt and "k_rp_com_tab" in lt and "k_rp_fixed_all" not in lt, sorted(lt)
    pinned = False
    for i in sorted(i for i in traced if i < len(proofs) and i not in (i_bad, i_neg, i_c)):
        tr = {}
        rp = zkat.RangeProof.deserialize(proofs[i])
        assert zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q, rounds, bits,
                              rp, tr) is None
        v, com, hp = _intermediates(pp, i)
        assert com == bn.g1_bytes(tr["com"]), i
        assert hp == [bn.g1_bytes(h) for h in tr["Hprime"]], i
        assert v[7] == tr["x0"], i
        if not pinned:  # the restatement used for the altered proofs is the oracle's
            assert _oracle_com(opp, rp, tr) == (tr["com"], tr["Hprime"])
            pinned = True
    for i in (i_neg, i_c):
        tr = {}
        rp = zkat.RangeProof.deserialize(proofs[i])
        err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q, rounds, bits,
                             rp, tr)
        assert err == "invalid range proof" and "com" not in tr
        c, hpo = _oracle_com(opp, rp, tr)
        _, com, hp = _intermediates(pp, i)
        assert com == bn.g1_bytes(c), i
        assert hp == [bn.g1_bytes(h) for h in hpo], i


@pytest.mark.parametrize("nhonest", [1, 63, 64, 65, 130])
def test_work_path_passes_8_bits(pp_raw, oracle_pp, nhonest):
    pp = _work_path_pp(pp_raw, 8)
    # the oracle traces the honest proofs at the pass's first position, around lane 64 and
    # at the last honest position (the malformed proof before it shifts it to nhonest)
    _run_pass(pp, oracle_pp.with_bit_length(8), 8, nhonest, {0, 62, 63, 64, nhonest}, seed=7 + nhonest)


def test_work_path_pass_64_bits(pp_raw, oracle_pp):
    pp = _work_path_pp(pp_raw, 64)
    _run_pass(pp, oracle_pp.with_bit_length(64), 64, 65, {0, 63, 64}, seed=64)
