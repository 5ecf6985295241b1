"""Generate tests/golden/idemix_audit_golden.json: idemix owner identities with the
audit information that opens (or fails to open) their EidNym / RhNym, each with the
verdict of the AuditInfo.Match restatement (tests/idemix_audit_ref.py).

The identities are made by the oracle's signer (oracle/idemix_identity.py sign) from
the reference's OWN credentials -- the SignerConfig / IssuerPublicKey fixtures in
tests/golden/idemix/ (charlie.ExtraId2: BN254; the zkatdlog validator's user:
FP256BN).  sign does not return the nyms' randomness, so the generator records the
draws of its random.Random: r_eid and r_rh are draws 13 and 14 (0-based) inside
sign, which the generator asserts by recomputing both commitments.  Synthetic cases
replace EidNym / RhNym with commitments to arbitrary strings; their proof no longer
verifies, which Match does not look at.

    python tests/golden/make_idemix_audit_golden.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import idemix as I, idemix_identity as ID, pairing as PR  # noqa: E402
import idemix_audit_ref as REF  # noqa: E402

OUT = os.path.join(HERE, "idemix_audit_golden.json")
CURVES = [("bn254", "bn254_charlie", I.BN254C, PR.BN254, 1), ("fp256bn", "fp256bn_validator", I.FP256BNC, PR.FP256BN, 0)]
ATTR_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 200)  # SHA-256 padding boundaries


class RecordingRandom(random.Random):
    """random.Random whose randrange keeps its results"""

    def __init__(self, seed):
        super().__init__(seed)
        self.draws = []

    def randrange(self, *a, **kw):
        v = super().randrange(*a, **kw)
        self.draws.append(v)
        return v


def _raw(*p):
    with open(os.path.join(HERE, "idemix", *p), "rb") as f:
        return f.read()


def cases(ipk, cred, eid, rh, C, PC, seed):
    rng = RecordingRandom(seed)
    HA, HR = ipk["h_attrs"], ipk["h_rand"]
    out = []

    def honest():
        rnym = rng.randrange(1, C.r)
        rng.draws = []
        sig, nym = ID.sign(ipk, cred, rnym, rng, PC)
        r_eid, r_rh = rng.draws[13], rng.draws[14]
        # a change in sign's order of draws fails here
        assert sig["EidNym"] == C.add(C.mul(HA[2], cred["attrs"][2]), C.mul(HR, r_eid))
        assert sig["RhNym"] == C.add(C.mul(HA[3], cred["attrs"][3]), C.mul(HR, r_rh))
        return sig, nym, r_eid, r_rh

    def commit(idx, attr, rand):
        return C.add(C.mul(HA[idx], C.hash_to_zr(attr)), C.mul(HR, rand))

    def add(name, sig, nym, eid_, r_eid_, rh_, r_rh_, proof=None, identity=None):
        if identity is None:
            p = ID.encode_signature(sig, PC) if proof is None else proof
            identity = ID.serialize_identity(C.g1_bytes(nym), p)
        out.append({"name": name, "identity": identity.hex(), "eid": eid_.hex(), "r_eid": "%064x" % r_eid_,
                    "rh": rh_.hex(), "r_rh": "%064x" % r_rh_})

    def off_curve(pt):
        return (pt[0], (pt[1] + 1) % C.p)

    def nym_field(f, point_proto, s):
        return I.pb_bytes_field(f, I.pb_bytes_field(1, point_proto) + I.pb_bytes_field(2, I.zr_bytes(s)))

    def without(proof, drop, extra=b""):
        """the proof's fields re-encoded without the field numbers in `drop`, then `extra`"""
        o = b""
        for f, wt, v in I.pb_fields(proof):
            if f not in drop:
                o += I.pb_bytes_field(f, v) if wt == 2 else ID._varint_field(f, v)
        return o + extra

    # ---- honest and scalar edges
    for k in range(3):
        s, n, re_, rr_ = honest()
        add("honest_%d" % k, s, n, eid, re_, rh, rr_)
    s, n, re_, rr_ = honest()
    add("r_eid_zero", dict(s, EidNym=commit(2, eid, 0)), n, eid, 0, rh, rr_)
    add("r_eid_equals_r", dict(s, EidNym=commit(2, eid, 0)), n, eid, C.r, rh, rr_)
    # ---- wrong openings and precedence
    add("wrong_eid", s, n, eid + b"x", re_, rh, rr_)
    add("wrong_r_eid", s, n, eid, (re_ + 1) % C.r, rh, rr_)
    add("wrong_rh", s, n, eid, re_, rh + b"x", rr_)
    add("wrong_r_rh", s, n, eid, re_, rh, (rr_ + 1) % C.r)
    add("both_wrong", s, n, eid + b"x", re_, rh + b"x", rr_)
    add("openings_swapped", s, n, rh, rr_, eid, re_)
    # ---- missing nyms
    add("no_eidnym", dict(s, EidNym=None), n, eid, re_, rh, rr_)
    add("no_rhnym", dict(s, RhNym=None), n, eid, re_, rh, rr_)
    add("no_eidnym_no_rhnym", dict(s, EidNym=None, RhNym=None), n, eid, re_, rh, rr_)
    full = ID.encode_signature(s, PC)
    add("eidnym_without_point", s, n, eid, re_, rh, rr_,
        proof=without(full, (18,), I.pb_bytes_field(18, I.pb_bytes_field(2, I.zr_bytes(s["sEid"])))))
    # ---- bad points
    add("eidnym_off_curve", dict(s, EidNym=off_curve(s["EidNym"])), n, eid, re_, rh, rr_)
    add("rhnym_off_curve", dict(s, RhNym=off_curve(s["RhNym"])), n, eid, re_, rh, rr_)
    add("rhnym_off_curve_eid_mismatch", dict(s, RhNym=off_curve(s["RhNym"])), n, eid + b"x", re_, rh, rr_)
    short = I.pb_bytes_field(1, s["EidNym"][0].to_bytes(32, "big")[1:]) + \
        I.pb_bytes_field(2, s["EidNym"][1].to_bytes(32, "big"))
    add("eidnym_31_byte_coordinate", s, n, eid, re_, rh, rr_,
        proof=without(full, (18,), nym_field(18, short, s["sEid"])))
    add("eidnym_all_zero", dict(s, EidNym=(0, 0)), n, eid, re_, rh, rr_)
    # ---- attribute lengths: both nyms commit to synthetic strings
    arng = random.Random(seed + 1000)
    for ln in ATTR_LENGTHS:
        a_eid, a_rh = bytes(arng.randrange(256) for _ in range(ln)), bytes(arng.randrange(256) for _ in range(ln))
        q_eid, q_rh = arng.randrange(1, C.r), arng.randrange(1, C.r)
        syn = dict(s, EidNym=commit(2, a_eid, q_eid), RhNym=commit(3, a_rh, q_rh))
        add("attr_len_%d" % ln, syn, n, a_eid, q_eid, a_rh, q_rh)
        if ln:  # the last byte changed (RH for the even lengths, EID for the odd ones)
            flip = lambda b: b[:-1] + bytes([b[-1] ^ 1])  # noqa: E731
            if ln % 2:
                add("attr_len_%d_last_byte" % ln, syn, n, flip(a_eid), q_eid, a_rh, q_rh)
            else:
                add("attr_len_%d_last_byte" % ln, syn, n, a_eid, q_eid, flip(a_rh), q_rh)
        else:  # the empty string against a one-byte one
            add("attr_len_0_last_byte", syn, n, b"\0", q_eid, a_rh, q_rh)
    # ---- proof parts that Match ignores
    add("tampered_sE", dict(s, sE=(s["sE"] + 1) % C.r), n, eid, re_, rh, rr_)
    add("bprime_off_curve", dict(s, BPrime=off_curve(s["BPrime"])), n, eid, re_, rh, rr_)
    if C is I.FP256BNC:  # malformed for the identity verifier (AMCL FromBytes reads 32 bytes)
        rest = b"".join(I.pb_bytes_field(f, v[1:] if f == 5 else v) if wt == 2 else ID._varint_field(f, v)
                        for f, wt, v in I.pb_fields(full))
        add("s_sk_31_bytes", s, n, eid, re_, rh, rr_, proof=rest)
    add("no_nym_public_key", s, n, eid, re_, rh, rr_, identity=I.pb_bytes_field(4, full))
    # ---- malformed inputs
    add("empty_identity", s, n, eid, re_, rh, rr_, identity=b"")
    add("empty_proof", s, n, eid, re_, rh, rr_, proof=b"")
    add("garbage_proof", s, n, eid, re_, rh, rr_, proof=b"\x0a\xff\xff")
    add("truncated_proof", s, n, eid, re_, rh, rr_, proof=full[:-7])
    add("field_5_varint", s, n, eid, re_, rh, rr_, proof=without(full, (5,), ID._varint_field(5, 7)))
    add("a_prime_garbage", s, n, eid, re_, rh, rr_, proof=without(full, (1,), I.pb_bytes_field(1, b"\x0a\xff\xff")))
    return out


def main():
    doc = {}
    for tag, d, C, PC, cid in CURVES:
        ipk = I.parse_ipk(_raw(d, "IssuerPublicKey"), C)
        sc = _raw(d, "SignerConfig")
        cred = ID.parse_signer_config(sc, C)
        eid, rh = REF.signer_strings(sc)
        cs = cases(ipk, cred, eid, rh, C, PC, seed=21 if cid else 22)
        for c in cs:
            c["error"] = REF.audit_match(ipk, C, bytes.fromhex(c["identity"]), bytes.fromhex(c["eid"]),
                                         int(c["r_eid"], 16), bytes.fromhex(c["rh"]), int(c["r_rh"], 16))
            print(tag, c["name"], c["error"], flush=True)
        doc[tag] = {"issuer": d, "curve_id": cid, "cases": cs}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
