"""CPU: the credential verifier's argument check and status strings (no device needed), the
second FP256BN credential fixture, and the bilinearity step the device path rests on --
e(W + g2 E, A) = e(g2, B)  <=>  e(W, A) e(g2, E A - B) = 1 -- on the oracle's pairing, for the
reference's credentials, a credential issued under the BN254 key whose secret the fixtures
hold, and its forgery 2 A."""
import hashlib
import random

import pytest

import cred_common as K
from oracle import idemix as OI, idemix_identity as ID

API_EINVAL = -1


def test_null_handle_is_einval():
    from fts_gpu import _lib as L
    import ctypes as C
    import numpy as np
    items = (L.CredItem * 1)()
    st = np.zeros(1, dtype=np.int32)
    stp = st.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.lib.fts_idemix_cred_verify_batch(None, 1, items, stp) == API_EINVAL
    assert L.lib.fts_idemix_cred_verify_batch(None, 0, None, None) == API_EINVAL
    assert L.lib.fts_idemix_cred_verify_last_timings(None, (C.c_float * 2)()) == API_EINVAL
    assert L.lib.fts_idemix_cred_verify_last_stats(None, (C.c_uint32 * 2)()) == API_EINVAL


def test_status_strings():
    from fts_gpu import _lib as L, idemix as I
    codes = (I.FTS_E_CRED_MALFORMED, I.FTS_E_CRED_B, I.FTS_E_CRED_PAIRING)
    # 35 stays unassigned: tests/test_sign_cpu.py pins fts_status_str(35) == "unknown status"
    assert codes == (36, 37, 38)
    s = [L.status_str(c) for c in codes]
    assert all(s) and len(set(s)) == 3 and "unknown" not in " ".join(s).lower()
    assert s[2] == "credential is not cryptographically valid" == I.message(38)
    assert L.status_str(34) not in s and L.status_str(39) == "unknown status"
    # every code from 35 to 37 has a non-empty string, all distinct
    t = [L.status_str(c) for c in (35, 36, 37)]
    assert all(t) and len(set(t)) == 3


def test_second_fp256bn_fixture():
    raw = K.raw("fp256bn_validator", "SignerConfig2")
    assert len(raw) == 663 and hashlib.sha256(raw).hexdigest().startswith("b91dcbef")
    ipk, _ = K.oracle_ipk("fp256bn_validator")
    a, b = K.signer("fp256bn_validator"), K.signer("fp256bn_validator", "SignerConfig2")
    assert a["A"] != b["A"]
    assert ID.credential_b(ipk, b) == b["B"]


def _items():
    rng = random.Random(20261021)
    issued = K.issue_bn254(rng)
    return [("bn254_charlie", K.signer("bn254_charlie"), True),
            ("fp256bn_validator", K.signer("fp256bn_validator"), True),
            ("fp256bn_validator", K.signer("fp256bn_validator", "SignerConfig2"), True),
            ("bn254_tokengen", issued, True),
            ("bn254_tokengen", dict(issued, A=OI.BN254C.mul(issued["A"], 2)), False)]


@pytest.mark.parametrize("k", range(5))
def test_rearranged_equation_equals_the_reference_form(k):
    issuer, cred, expect = _items()[k]
    ipk, W = K.oracle_ipk(issuer)
    assert ID.credential_b(ipk, cred) == cred["B"]
    assert ID.credential_pairing_ok(K.ISSUERS[issuer][2], W, cred) is expect
    assert K.rearranged_ok(issuer, W, cred) is expect
