"""CPU: the issuer key's proof of knowledge restated on the oracle curves
(tests/issuer_key_ref.py: the reference the GPU tests compare with), pinned by the reference's
four issuer keys; the host side of the issuer-key calls (csrc/host/ipk_write.hpp) through the
library's host-only entry points and lib/ipk_check (a stand-alone program built with the host
address and undefined-behaviour sanitizers)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from conftest import PKG

import cred_issue_ref as R
import issuer_key_ref as K

KEYS = [(tag, name) for tag in ("bn254", "fp256bn") for name in K.GOLDEN_KEYS[tag]]


@pytest.fixture(scope="module")
def parts():
    """(tag, issuer) -> (c, the six transcript points) of the golden key, computed once"""
    return {(tag, name): K.proof_parts(tag, K.golden(name)) for tag, name in KEYS}


@pytest.mark.parametrize("tag,name", KEYS)
def test_golden_keys_verify_in_proto_order_only(tag, name, parts):
    """all four keys of the reference verify with the G2 points hashed as the ECP2 proto's four
    coordinates in field order, on both curves, and under no other order of the four"""
    c, pts = parts[(tag, name)]
    assert K.challenge(tag, pts) == c
    assert K.check(tag, K.golden(name)) == K.OK
    for order in itertools.permutations(range(4)):
        if order != (0, 1, 2, 3):
            assert K.challenge(tag, pts, order) != c, order


@pytest.mark.parametrize("tag,name", KEYS)
def test_stored_hash_is_the_hash_without_it(tag, name):
    raw = K.golden(name)
    assert K.stored_hash(raw) == K.hash_of(tag, raw)
    assert len(raw) == 843


@pytest.mark.parametrize("tag,name", KEYS)
def test_mutated_proofs_fail(tag, name):
    """ProofC + 1, ProofS + 1, W replaced by 2 W, BarG1 and BarG2 swapped: the proof fails"""
    want = {"proof_c+1", "proof_s+1", "w->2w", "barg1<->barg2"}
    seen = set()
    for nm, raw, expect in K.mutants(tag, K.golden(name)):
        if nm in want:
            seen.add(nm)
            assert expect == K.PROOF and K.check(tag, raw) == K.PROOF, nm
    assert seen == want


def test_restatement_verdicts_of_every_mutant():
    """the restatement gives each of the issue's mutants the status the header names (one key per
    curve: the GPU tests compare the device with these verdicts)"""
    for tag in ("bn254", "fp256bn"):
        ms = K.mutants(tag, K.golden(K.GOLDEN_KEYS[tag][0]))
        names = [m[0] for m in ms]
        # + r fits 32 bytes on BN254 (r < 2^254); on FP256BN 2^256 - r is below 2^209
        assert ("proof_s+r" in names) == ("proof_c+r" in names) == (tag == "bn254")
        assert len(names) == (17 if tag == "bn254" else 15) and "barg2 identity" in names
        for nm, raw, expect in ms:
            assert K.check(tag, raw) == expect, (tag, nm)


def test_status_codes_and_strings():
    from fts_gpu import _lib as L, idemix as I
    assert (I.FTS_E_IPK_MALFORMED, I.FTS_E_IPK_UNDEFINED, I.FTS_E_IPK_PROOF) == (43, 44, 45) == \
        (K.MALFORMED, K.UNDEFINED, K.PROOF)
    assert L.status_str(44) == "some part of the public key is undefined"
    assert L.status_str(45) == "zero knowledge proof in public key invalid"
    assert L.status_str(43) != "unknown status" and L.status_str(46) == "unknown status"
    assert I.FTS_IDEMIX_IPK_LEN == 843


def test_host_part_of_the_check():
    """what the host decides before the device runs (parse, missing parts, lengths) and the hash"""
    from fts_gpu import idemix as I
    for tag in ("bn254", "fp256bn"):
        cid = R.CURVES[tag][0]
        for name in K.GOLDEN_KEYS[tag]:
            raw = K.golden(name)
            assert I.parse_issuer_key(cid, raw) == (K.OK, K.stored_hash(raw))
        raw = K.golden(K.GOLDEN_KEYS[tag][0])
        host_decides = {"no barg1", "no hrand", "one hattrs fewer", "31-byte proof_c", "truncated", "empty"}
        for nm, m, expect in K.mutants(tag, raw):
            st, h = I.parse_issuer_key(cid, m)
            assert st == (expect if nm in host_decides else K.OK), (tag, nm)
            if nm not in ("truncated", "empty"):
                assert h == K.hash_of(tag, m), (tag, nm)
        assert I.parse_issuer_key(cid, None)[0] == K.MALFORMED
        # the hash leaves out field 10 wherever it stands, and only it
        moved = K.rebuild([f for f in K.fields(raw) if f[0] == 10] + [f for f in K.fields(raw) if f[0] != 10])
        assert I.parse_issuer_key(cid, moved) == (K.OK, K.stored_hash(raw))


def test_keygen_draws():
    """ten values in [1, r), stable for a seed, different between i and i + 1, refused for the
    secure source"""
    from fts_gpu import _lib as L, idemix as I
    for tag in ("bn254", "fp256bn"):
        cid, Cv, _ = R.CURVES[tag]
        for seed in (0, 7, (1 << 63) + 5):
            d = I.keygen_draws(cid, seed, 3)
            assert len(d) == 10 and all(1 <= v < Cv.r for v in d) and len(set(d)) == 10
            assert d == I.keygen_draws(cid, seed, 3) == I.keygen_draws(cid, seed + 3, 0)
            nxt = I.keygen_draws(cid, seed, 4)
            assert all(a != b for a, b in zip(d, nxt))
        with pytest.raises(L.FtsError) as e:
            I.keygen_draws(cid, L.FTS_SEED_OS_RANDOM, 0)
        assert e.value.code == -1
    assert L.lib.fts_debug_idemix_keygen_draws(7, 1, 0, (C.c_uint8 * 320)()) == -1
    assert L.lib.fts_debug_idemix_keygen_draws(1, 1, 0, None) == -1


def test_api_argument_codes():
    """the return codes that need no device: n = 0, NULL arrays, n > 2^22, an unknown curve, a
    stride below the key's length"""
    from fts_gpu import _lib as L
    chk, gen = L.lib.fts_idemix_ipk_check_batch, L.lib.fts_idemix_issuer_keygen_batch
    ptrs, lens, st = (C.c_void_p * 1)(), (C.c_size_t * 1)(), (C.c_int32 * 1)()
    assert chk(0, 1, 0, None, None, None, None) == 0
    assert chk(0, 1, 1, None, lens, st, None) == chk(0, 1, 1, ptrs, None, st, None) == -1
    assert chk(0, 1, 1, ptrs, lens, None, None) == -1
    assert chk(0, 1, (1 << 22) + 1, ptrs, lens, st, None) == -1
    assert chk(0, 5, 1, ptrs, lens, st, None) == chk(0, 5, 0, None, None, None, None) == -1
    isk, out, ln = (C.c_uint8 * 32)(), (C.c_uint8 * 843)(), (C.c_uint32 * 1)()
    assert gen(0, 1, 0, 1, None, None, 0, None) == 0
    assert gen(0, 1, 1, 1, None, out, 843, ln) == gen(0, 1, 1, 1, isk, None, 843, ln) == -1
    assert gen(0, 1, 1, 1, isk, out, 843, None) == gen(0, 3, 1, 1, isk, out, 843, ln) == -1
    assert gen(0, 0, (1 << 22) + 1, 1, isk, out, 843, ln) == -1
    esize = -5  # FTS_API_ESIZE, before a byte is written
    assert gen(0, 1, 1, 1, isk, out, 842, ln) == gen(0, 0, 1, 1, isk, out, 0, ln) == esize
    assert bytes(out) == bytes(843) and bytes(isk) == bytes(32)
    assert L.lib.fts_idemix_issuer_key_last_timings(None) == -1


def test_ipk_check_program():
    """lib/ipk_check (csrc/tools/ipk_check.cpp): the check's reading of a key on the four fixtures
    and on a written key (truncations at every length, length-field overflows, repeated and
    missing fields, 31- and 33-byte coordinates), the hash, the writer, the draws, under the host
    sanitizers"""
    args = ["%s:%s" % (tag, os.path.join(R.GOLD, name, "IssuerPublicKey")) for tag, name in KEYS]
    out = subprocess.run([os.path.join(PKG, "lib", "ipk_check")] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ipk_check: ok (4 fixture keys)" in out.stdout
