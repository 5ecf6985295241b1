"""GPU: idemix audit info matched against owner identities on the device
(fts_idemix_audit_match_batch, k_idv_audit) against the verdicts of the
AuditInfo.Match restatement (tests/idemix_audit_ref.py) stored in
tests/golden/idemix_audit_golden.json, on both curves: the golden cases, the
half-major lane mapping at batch sizes around one wave, agreement with the
identity verifier on one handle, another issuer's key, nil rands, concurrent calls
and the timing getter."""
import json
import os
import random
import threading

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = pytest.mark.gpu
TAGS = ["bn254", "fp256bn"]


def _load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def _ipk(d):
    with open(os.path.join(GOLD, "idemix", d, "IssuerPublicKey"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def doc():
    return _load("idemix_audit_golden.json")


@pytest.fixture(scope="module")
def verifiers(doc):
    from fts_gpu import idemix as I
    vs = {tag: I.IdentityVerifier(_ipk(doc[tag]["issuer"]), device=0, curve=doc[tag]["curve_id"]) for tag in TAGS}
    yield vs
    for v in vs.values():
        v.close()


def _args(cases):
    """the five parallel lists of audit_match_batch"""
    return ([bytes.fromhex(c["identity"]) for c in cases], [bytes.fromhex(c["eid"]) for c in cases],
            [bytes.fromhex(c["r_eid"]) for c in cases], [bytes.fromhex(c["rh"]) for c in cases],
            [bytes.fromhex(c["r_rh"]) for c in cases])


def _messages(st):
    from fts_gpu import idemix as I
    return [I.message(int(s)) for s in st]


@pytest.mark.parametrize("tag", TAGS)
def test_golden_verdicts(verifiers, doc, tag):
    cases = doc[tag]["cases"]
    st = verifiers[tag].audit_match_batch(*_args(cases))
    assert dict(zip((c["name"] for c in cases), _messages(st))) == {c["name"]: c["error"] for c in cases}


@pytest.mark.parametrize("tag", TAGS)
def test_lane_mapping(doc, tag):
    """257, 1, 65, 64, 63 items on one fresh handle (the slot's buffers grow, then are
    reused by smaller calls); 65 and 63 put EID and RH lanes into one wave, 257 spreads
    each half over more than one block; every status at its position"""
    from fts_gpu import idemix as I
    cases = doc[tag]["cases"]
    rng = random.Random(5)
    v = I.IdentityVerifier(_ipk(doc[tag]["issuer"]), device=0, curve=doc[tag]["curve_id"])
    try:
        for n in (257, 1, 65, 64, 63):
            pick = [cases[rng.randrange(len(cases))] for _ in range(n)]
            st = v.audit_match_batch(*_args(pick))
            assert _messages(st) == [c["error"] for c in pick], n
            if n == 65:
                assert (v.audit_match_batch(*_args(pick)) == st).all()
    finally:
        v.close()


@pytest.mark.parametrize("tag", TAGS)
def test_agrees_with_identity_verifier_on_one_handle(verifiers, doc, tag):
    """honest identities pass the proof check and the match; a tampered proof fails the
    first and still matches (Match does not verify the proof)"""
    from fts_gpu import idemix as I
    by = {c["name"]: c for c in doc[tag]["cases"]}
    names = ["honest_0", "honest_1", "honest_2", "tampered_sE"]
    cs = [by[n] for n in names]
    V = verifiers[tag]
    assert [int(s) for s in V.verify_batch([bytes.fromhex(c["identity"]) for c in cs])] == [0, 0, 0, I.FTS_E_ID_ZK]
    assert [int(s) for s in V.audit_match_batch(*_args(cs))] == [0, 0, 0, 0]
    V.Match(*[a[0] for a in _args(cs[:1])])
    with pytest.raises(I.AuditMatchError, match="eid nym does not match") as e:
        V.Match(*[a[0] for a in _args([by["wrong_eid"]])])
    assert e.value.status == I.FTS_E_AUDIT_EID_MISMATCH


ATTR_LENS = [0, 1, 3, 4, 55, 56, 63, 64, 65, 119, 120, 127, 128]


@pytest.mark.parametrize("tag", TAGS)
def test_attribute_lengths_around_the_block_edges(verifiers, doc, tag):
    """one batch whose eid / rh strings have the lengths where the padded stream's words
    change shape (a partial last word, the terminator in a word of its own, the bit
    length in a further block; the golden cases lack 3, 4, 127 and 128): honest_0 with
    both nyms committing to synthetic strings, the eid's length ascending and the rh's
    descending, then the same with the last byte of the longer string flipped; every
    verdict is AuditInfo.Match's (tests/idemix_audit_ref.py)"""
    import idemix_audit_ref as REF
    from oracle import idemix as OI
    C = OI.CURVES[doc[tag]["curve_id"]]
    ipk = OI.parse_ipk(_ipk(doc[tag]["issuer"]), C)
    base = bytes.fromhex(next(c for c in doc[tag]["cases"] if c["name"] == "honest_0")["identity"])
    outer = OI.pb_fields(base)
    proof = OI.pb_fields(OI._pb_bytes(outer, 4))
    rng = random.Random(128)

    def with_nyms(points):
        """the identity with the points of fields 18 / 19 replaced (their responses kept)"""
        p = b""
        for f, wt, v in proof:
            assert wt == 2 or f == 16
            if f in points:
                x, y = points[f]
                ecp = OI.pb_bytes_field(1, x.to_bytes(32, "big")) + OI.pb_bytes_field(2, y.to_bytes(32, "big"))
                v = OI.pb_bytes_field(1, ecp) + OI.pb_bytes_field(2, OI._pb_bytes(OI.pb_fields(v), 2))
            p += OI.pb_bytes_field(f, v) if wt == 2 else REF.ID._varint_field(f, v)
        return b"".join(OI.pb_bytes_field(f, p if f == 4 else v) for f, _, v in outer)

    items = []
    for le, lr in zip(ATTR_LENS, reversed(ATTR_LENS)):
        eid, rh = rng.randbytes(le), rng.randbytes(lr)
        q_eid, q_rh = rng.randrange(1, C.r), rng.randrange(1, C.r)
        pts = {18: C.add(C.mul(ipk["h_attrs"][2], C.hash_to_zr(eid)), C.mul(ipk["h_rand"], q_eid)),
               19: C.add(C.mul(ipk["h_attrs"][3], C.hash_to_zr(rh)), C.mul(ipk["h_rand"], q_rh))}
        ident = with_nyms(pts)
        items.append((ident, eid, q_eid, rh, q_rh))
        flip = lambda b: b[:-1] + bytes([b[-1] ^ 1])  # noqa: E731
        items.append((ident, flip(eid), q_eid, rh, q_rh) if le >= lr else (ident, eid, q_eid, flip(rh), q_rh))
    want = [REF.audit_match(ipk, C, *it) for it in items]
    assert want[0::2] == [None] * len(ATTR_LENS)
    assert set(want[1::2]) == {REF.E_EID_MISMATCH, REF.E_RH_MISMATCH}
    st = verifiers[tag].audit_match_batch([it[0] for it in items], [it[1] for it in items],
                                          [it[2].to_bytes(32, "big") for it in items], [it[3] for it in items],
                                          [it[4].to_bytes(32, "big") for it in items])
    assert _messages(st) == want


def test_wrong_issuer(doc):
    """charlie's honest BN254 identities under the tokengen issuer key: other bases, so
    the first commitment already differs"""
    from fts_gpu import idemix as I
    other = I.IdentityVerifier(_ipk("bn254_tokengen"), device=0, curve=I.FTS_CURVE_BN254)
    try:
        cs = [c for c in doc["bn254"]["cases"] if c["name"].startswith("honest_")]
        assert len(cs) == 3
        assert [int(s) for s in other.audit_match_batch(*_args(cs))] == [I.FTS_E_AUDIT_EID_MISMATCH] * 3
    finally:
        other.close()


@pytest.mark.parametrize("tag", TAGS)
def test_null_rands_and_null_empty_attribute(verifiers, doc, tag):
    from fts_gpu import idemix as I
    by = {c["name"]: c for c in doc[tag]["cases"]}
    cs = [by[n] for n in ("honest_0", "honest_1", "wrong_rh", "honest_2", "attr_len_0")]
    ids, eids, r_eids, rhs, r_rhs = _args(cs)
    r_eids[1] = None
    r_rhs[3] = None
    assert eids[4] == b"" and rhs[4] == b""
    eids[4] = None  # eid = NULL, eid_len = 0: the empty string
    st = verifiers[tag].audit_match_batch(ids, eids, r_eids, rhs, r_rhs)
    assert [int(s) for s in st] == [0, I.FTS_E_AUDIT_MALFORMED, I.FTS_E_AUDIT_RH_MISMATCH, I.FTS_E_AUDIT_MALFORMED, 0]


@pytest.mark.parametrize("tag", TAGS)
def test_concurrent_calls_on_one_handle(verifiers, doc, tag):
    """four threads x three match calls of 65 items beside one thread verifying the
    64-identity tile, all on one handle: every result equals the same call made alone"""
    V = verifiers[tag]
    cases = doc[tag]["cases"]
    tile = [bytes.fromhex(t["identity"]) for t in _load("idemix_identity_golden.json")[tag]["tile"]]
    rng = random.Random(17)
    batches = [_args([cases[rng.randrange(len(cases))] for _ in range(65)]) for _ in range(4)]
    alone = [V.audit_match_batch(*b) for b in batches]
    tile_alone = V.verify_batch(tile)
    got, errors = {}, []

    def match(k):
        try:
            got[k] = [V.audit_match_batch(*batches[k]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def verify():
        try:
            got["tile"] = V.verify_batch(tile)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=match, args=(k,)) for k in range(4)] + [threading.Thread(target=verify)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    for k in range(4):
        assert all((r == alone[k]).all() for r in got[k])
    assert (got["tile"] == tile_alone).all()


@pytest.mark.parametrize("tag", TAGS)
def test_timing_and_empty_batch(verifiers, doc, tag):
    V = verifiers[tag]
    st = V.audit_match_batch(*_args(doc[tag]["cases"][:3]))
    assert len(st) == 3 and V.last_audit_kernel_ms() > 0
    empty = V.audit_match_batch([])
    assert isinstance(empty, np.ndarray) and empty.dtype == np.int32 and len(empty) == 0
