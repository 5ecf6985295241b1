"""CPU: the host side of idemix enrolment (csrc/host/credreq_write.hpp) through the library's
host-only entry points and lib/credissue_check (a stand-alone program built with the host
address and undefined-behaviour sanitizers), and the restatement the GPU tests compare with
(tests/cred_issue_ref.py): its credentials satisfy the oracle's Credential.Ver under the
reference's own BN254 issuer secret and under a made FP256BN key."""
import os
import random
import subprocess

import pytest

from conftest import PKG

import cred_issue_ref as R
from oracle import idemix as OI, idemix_identity as ID

TAGS = ["bn254", "fp256bn"]


def _key(tag):
    """-> (isk, IssuerPublicKey proto): the reference's own on BN254, a made one on FP256BN"""
    return R.tokengen() if tag == "bn254" else R.make_issuer_key(tag, random.Random(4100))


@pytest.mark.parametrize("tag", TAGS)
def test_fast_mul_equals_the_oracle_curve(tag):
    _, C, _ = R.CURVES[tag]
    rng = random.Random(7)
    pt = C.mul(R.G1, rng.randrange(C.r))
    for k in (0, 1, 2, 3, C.r - 1, C.r, C.r + 5, rng.randrange(C.r), rng.randrange(C.r)):
        assert R.mul(C, pt, k) == C.mul(pt, k)
    assert R.mul(C, None, 5) is None


@pytest.mark.parametrize("tag", TAGS)
def test_restated_credentials_satisfy_credential_ver(tag):
    _, C, PC = R.CURVES[tag]
    isk, raw = _key(tag)
    ipk, W = OI.parse_ipk(raw, C), ID.ipk_w(PC, raw)
    rng = random.Random(11)
    sk, nonce = rng.randrange(C.r), rng.randbytes(32)
    req = R.new_cred_request(ipk, sk, nonce, rng.randrange(C.r))
    assert len(req) == 172 and R.check_request(ipk, req) == R.OK
    k = R.new_credential(ipk, isk, req, [0, 1, C.r - 1, rng.randrange(C.r)], rng.randrange(C.r), rng.randrange(C.r))
    k["sk"] = sk
    assert ID.credential_b(ipk, k) == k["B"]
    assert ID.credential_pairing_ok(PC, W, k)
    assert len(R.cred_proto(k)) == 344
    # the pairing check discriminates: another secret's credential is not valid
    bad = dict(R.new_credential(ipk, isk + 1, req, k["attrs"], k["E"], k["S"]), sk=sk)
    assert ID.credential_b(ipk, bad) == bad["B"] and not ID.credential_pairing_ok(PC, W, bad)
    # the request's verdicts
    f = OI.pb_fields(req)
    c, s = (int.from_bytes(OI._pb_bytes(f, q), "big") for q in (3, 4))
    nym = R._parse_request(ipk, req)[0]
    assert R.check_request(ipk, R.encode_request(nym, nonce, c, (s + 1) % C.r)) == R.INVALID
    if c + C.r < 1 << 256:
        assert R.check_request(ipk, R.encode_request(nym, nonce, c + C.r, s)) == R.INVALID
    if s + C.r < 1 << 256:
        assert R.check_request(ipk, R.encode_request(nym, nonce, c, s + C.r)) == R.OK
    assert R.check_request(ipk, R.encode_request((nym[0], (nym[1] + 1) % C.p), nonce, c, s)) == R.MALFORMED
    assert R.check_request(ipk, req[:-1]) == R.MALFORMED and R.check_request(ipk, b"") == R.MALFORMED


@pytest.mark.parametrize("tag", TAGS)
def test_made_key_parses_and_proves(tag):
    _, C, PC = R.CURVES[tag]
    isk, raw = R.make_issuer_key(tag, random.Random(4200))
    ipk = OI.parse_ipk(raw, C)
    assert len(ipk["h_attrs"]) == 4 and len(ipk["attribute_names"]) == 4
    assert ipk["bar_g2"] == C.mul(ipk["bar_g1"], isk)
    assert ID.ipk_w(PC, raw) == PC.g2_mul(PC.g2_gen, isk)
    assert ipk["hash"] == OI.zr_bytes(C.hash_to_zr(OI.ipk_hash_input(raw)))
    if tag == "bn254":
        assert OI.ipk_proof_valid(ipk)
    # the reference's own secret against its own key, the relation an issuer handle checks
    risk, rraw = R.tokengen()
    rk = OI.parse_ipk(rraw, OI.BN254C)
    assert rk["bar_g2"] == R.mul(OI.BN254C, rk["bar_g1"], risk)


def test_exported_lengths_and_statuses():
    from fts_gpu import _lib as L, idemix as I
    assert (I.FTS_IDEMIX_CRED_REQUEST_LEN, I.FTS_IDEMIX_CREDENTIAL_LEN) == (172, 344)
    with open(os.path.join(os.path.dirname(PKG), "include", "fts_gpu.h")) as f:
        h = f.read()
    assert "#define FTS_IDEMIX_CRED_REQUEST_LEN 172" in h and "#define FTS_IDEMIX_CREDENTIAL_LEN 344" in h
    # 39 stays unassigned (tests/test_cred_verify_cpu.py pins fts_status_str(39) == "unknown status")
    assert (I.FTS_E_CREDREQ_MALFORMED, I.FTS_E_CREDREQ_INVALID) == (40, 41) == (R.MALFORMED, R.INVALID)
    assert L.status_str(40) == "one of the proof values is undefined"
    assert L.status_str(41) == "zero knowledge proof is invalid"
    assert L.status_str(39) == L.status_str(42) == "unknown status"


@pytest.mark.parametrize("tag", TAGS)
def test_writers_and_parser_equal_the_restatement(tag):
    from fts_gpu import idemix as I
    cid, C, _ = R.CURVES[tag]
    isk, raw = _key(tag)
    ipk = OI.parse_ipk(raw, C)
    rng = random.Random(23 + cid)
    for sk in (1, C.r - 1, rng.randrange(C.r)):
        nonce = rng.randbytes(32)
        req = R.new_cred_request(ipk, sk, nonce, rng.randrange(C.r))
        nym, _, c, s = R._parse_request(ipk, req)
        assert I.write_cred_request(nym, nonce, c, s) == req and len(req) == I.FTS_IDEMIX_CRED_REQUEST_LEN
        assert I.parse_cred_request(cid, req) == (R.OK, ID.ecp(nym)[2:34] + ID.ecp(nym)[36:], nonce, c, s)
        k = R.new_credential(ipk, isk, req, [0, 1, C.r - 1, rng.randrange(C.r)], rng.randrange(C.r), rng.randrange(C.r))
        got = I.write_credential(k["A"], k["B"], k["E"], k["S"], k["attrs"])
        assert got == R.cred_proto(k) and len(got) == I.FTS_IDEMIX_CREDENTIAL_LEN
    # the parser's part of the verdicts: unreduced scalars, lengths, wire types, missing fields
    big = (1 << 256) - 1
    st, _, _, cc, ss = I.parse_cred_request(cid, R.encode_request(nym, nonce, big, big))
    assert (st, cc, ss) == (R.OK, big, big % C.r)
    f = OI.pb_fields(req)
    for drop in (1, 2, 3, 4):
        cut = b"".join(OI.pb_bytes_field(q, v) for q, _, v in f if q != drop)
        assert I.parse_cred_request(cid, cut)[0] == R.MALFORMED
    for bad in (R.encode_request(nym, nonce[:31], c, s), R.encode_request(nym, nonce + b"\0", c, s),
                R.encode_request(nym, nonce, OI.zr_bytes(c)[1:], s), R.encode_request(nym, nonce, c, b"\0" + OI.zr_bytes(s)),
                req[:-1], req + b"\x18\x05", b"", None):
        assert I.parse_cred_request(cid, bad)[0] == R.MALFORMED
    # repeated and unknown fields: the last occurrence wins, the rest is skipped
    again = req + OI.pb_bytes_field(3, R.z32(7)) + OI.pb_bytes_field(9, b"xyz") + b"\x53\x08\x01\x54"
    assert I.parse_cred_request(cid, again)[:4] == (R.OK, ID.ecp(nym)[2:34] + ID.ecp(nym)[36:], nonce, 7)


@pytest.mark.parametrize("tag", TAGS)
def test_draws_deterministic_distinct_below_r(tag):
    from fts_gpu import idemix as I, _lib as L
    cid, C, _ = R.CURVES[tag]
    for seed in (0, 1, 77, (1 << 63) + 5):
        d = [I.cred_issue_draws(cid, seed, i) for i in range(6)]
        assert d == [I.cred_issue_draws(cid, seed, i) for i in range(6)]
        for E, S, rsk in d:
            assert 0 <= E < C.r and 0 <= S < C.r and E != S and rsk == E  # either call's first draw
        for i in range(5):
            assert not set(d[i]) & set(d[i + 1])
            assert d[i + 1] == I.cred_issue_draws(cid, seed + 1, i)  # item i + 1 is item i at seed + 1
        # an avoided first E: the item's second draw becomes E, its third S
        E, S, rsk = d[0]
        E2, S2, rsk2 = I.cred_issue_draws(cid, seed, 0, avoid_e=E)
        assert E2 == S and S2 not in (E, S) and S2 < C.r and rsk2 == rsk
        assert I.cred_issue_draws(cid, seed, 0, avoid_e=(E + 1) % C.r) == d[0]
    with pytest.raises(L.FtsError):
        I.cred_issue_draws(cid, (1 << 64) - 1, 0)
    with pytest.raises(L.FtsError):
        I.cred_issue_draws(2, 1, 0)


def test_null_handles_and_arguments():
    import ctypes as C
    import numpy as np
    from fts_gpu import _lib as L
    st = np.zeros(1, dtype=np.int32)
    stp = st.ctypes.data_as(C.POINTER(C.c_int32))
    buf = (C.c_uint8 * 344)()
    ln = (C.c_uint32 * 1)()
    assert L.lib.fts_idemix_cred_request_batch(None, 1, bytes(32), bytes(32), 1, buf, 172, ln, stp) == -1
    assert L.lib.fts_idemix_cred_request_verify_batch(None, 0, None, None) == -1
    assert L.lib.fts_idemix_cred_request_last_timings(None, (C.c_float * 2)()) == -1
    h = C.c_void_p(1)
    assert L.lib.fts_idemix_issuer_create(None, bytes(32), C.byref(h)) == -1 and not h.value
    assert L.lib.fts_idemix_cred_issue_batch(None, 1, (L.CredIssueItem * 1)(), 1, buf, 344, ln, stp) == -1
    assert L.lib.fts_idemix_cred_issue_last_timings(None, (C.c_float * 2)(), None) == -1
    L.lib.fts_idemix_issuer_destroy(None)


def test_credissue_check_program():
    """lib/credissue_check (csrc/tools/credissue_check.cpp): the request parser on honest and
    mutated requests (truncations, over-long fields, varint overflow, repeated and unknown
    fields, groups), the writers round-tripped, the draws, under the host sanitizers"""
    out = subprocess.run([os.path.join(PKG, "lib", "credissue_check")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "credissue_check: ok" in out.stdout
