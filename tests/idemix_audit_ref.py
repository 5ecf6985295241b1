"""AuditInfo.Match for idemix owner identities, restated in pure Python.  TEST
INFRASTRUCTURE ONLY: never imported by the product path.

Reference call chain (fabric-token-sdk):
* crypto/audit/auditor.go:225-282  InspectOutput / InspectInputs call
  matcher.MatchIdentity for every output, input and issuer
* services/identity/idemix/crypto/audit.go:40-84  AuditInfo.Match(id):
  proto.Unmarshal(id, SerializedIdemixIdentity), then two Csp.Verify calls on
  serialized.Proof with EidNymAuditOpts{EidIndex 2, string(Attributes[2]),
  EidNymAuditData.Rand} and RhNymAuditOpts{RhIndex 3, string(Attributes[3]),
  RhNymAuditData.Rand}, audit type AuditExpectSignature (the zero value)
* IBM/idemix (v0.0.2-0.20240816143710-3dce4618d760, NOT vendored: restated from
  the published bccsp handlers and signature.go) Signature.AuditNymEid /
  AuditNymRh: the signature must not be empty and must unmarshal; nil EidNym or
  EidNym.Nym -> "no EidNym provided"; EidNym' = HAttrs[2].Mul2(HashToZr(eid),
  HRand, RNymEid); G1FromProto(sig.EidNym.Nym); "eid nym does not match"

UNPINNED, in the same sense as the identity proof's transcript in
oracle/idemix_identity.py: no audit vector exists in the reference.  PINNED: the
attribute encoding HashToZr(string) by the SignerConfig fixtures
(tests/test_idemix_audit_cpu.py), HashToZr and the G1 encodings by the
IssuerPublicKey fixtures.

The proof is NOT verified: no other point of the signature is decoded and no
scalar parsed, but proto.Unmarshal validates the wire format of the whole
Signature, embedded messages included.  The wire is walked here (oracle.idemix
pb_fields), not through oracle.idemix_identity.decode_signature, which parses
scalars.  The strings are those of the library's fts_status_str: one per status,
so the several ways an identity fails to deserialize share one message.
"""
from oracle import idemix as I
from oracle import idemix_identity as ID

E_MALFORMED = "could not deserialize the identity, its proof or the audit data"
E_NO_EIDNYM = "error while verifying the nym eid: no EidNym provided"
E_EID_POINT = "error while verifying the nym eid: invalid EidNym point"
E_EID_MISMATCH = "error while verifying the nym eid: eid nym does not match"
E_NO_RHNYM = "error while verifying the nym rh: no RhNym provided"
E_RH_POINT = "error while verifying the nym rh: invalid RhNym point"
E_RH_MISMATCH = "error while verifying the nym rh: rh nym does not match"
# fts_status numbering (include/fts_gpu.h)
STATUS = {None: 0, E_MALFORMED: 27, E_NO_EIDNYM: 28, E_EID_POINT: 29, E_EID_MISMATCH: 30, E_NO_RHNYM: 31,
          E_RH_POINT: 32, E_RH_MISMATCH: 33}


def signer_strings(raw):
    """(enrollment_id, revocation_handle) of an IdemixSignerConfig (JSON or proto)"""
    import json
    try:
        j = json.loads(raw)
        return j["enrollment_id"].encode(), j["revocation_handle"].encode()
    except (ValueError, UnicodeDecodeError):
        f = I.pb_fields(raw)
        return I._pb_bytes(f, 5), I._pb_bytes(f, 7)


class _Wire(ValueError):
    pass


def _msg(raw, bytes_fields, varint_fields=()):
    """fields of one message; a known field with another wire type fails Unmarshal"""
    f = I.pb_fields(raw)
    for ff, wt, _ in f:
        if (ff in bytes_fields and wt != 2) or (ff in varint_fields and wt != 0):
            raise _Wire("field %d: wire type %d" % (ff, wt))
    return f


class _Ecp:
    """ECP{1 x, 2 y}; proto3 merges the occurrences of an embedded message field"""

    def __init__(self):
        self.x = self.y = b""

    def merge(self, raw):
        for ff, _, v in _msg(raw, (1, 2)):
            if ff == 1:
                self.x = v
            if ff == 2:
                self.y = v

    def proto(self):
        return I.pb_bytes_field(1, self.x) + I.pb_bytes_field(2, self.y)


def unmarshal_nyms(proof):
    """proto.Unmarshal(proof, idemix.Signature) as far as Match needs it: the whole
    wire format checked, -> (EidNym.Nym, RhNym.Nym) as _Ecp or None (nil)"""
    nyms = {18: None, 19: None}
    for ff, wt, v in _msg(proof, [k for k in range(1, 20) if k != 16], (16,)):
        if ff in (1, 2, 3, 12):
            _Ecp().merge(v)
        elif ff == 14:
            _msg(v, (1, 2, 3, 4))
        elif ff == 17:
            _msg(v, (2,), (1,))
        elif ff in (18, 19):
            for sf, _, sv in _msg(v, (1, 2)):
                if sf == 1:
                    if nyms[ff] is None:
                        nyms[ff] = _Ecp()
                    nyms[ff].merge(sv)
    return nyms[18], nyms[19]


def audit_match(ipk, C, identity, eid, r_eid, rh, r_rh):
    """AuditInfo.Match -> None or the error string.  ipk: oracle.idemix.parse_ipk;
    eid / rh: the attribute strings (bytes); r_eid / r_rh: the rands (int, used mod r)"""
    try:
        proof = I._pb_bytes(_msg(identity, (1, 2, 3, 4)), 4)
        if not proof:  # bccsp: "invalid signature, it must not be empty"
            return E_MALFORMED
        eid_nym, rh_nym = unmarshal_nyms(proof)
    except ValueError:
        return E_MALFORMED
    halves = ((eid_nym, 2, eid, r_eid, E_NO_EIDNYM, E_EID_POINT, E_EID_MISMATCH),
              (rh_nym, 3, rh, r_rh, E_NO_RHNYM, E_RH_POINT, E_RH_MISMATCH))
    for nym, idx, attr, rand, e_nil, e_point, e_mismatch in halves:
        if nym is None:
            return e_nil
        want = C.add(C.mul(ipk["h_attrs"][idx], C.hash_to_zr(attr)), C.mul(ipk["h_rand"], rand % C.r))
        try:
            got = ID._g1_proto(C, nym.proto())
        except (ValueError, I.PointError):
            return e_point
        if want != got:
            return e_mismatch
    return None
