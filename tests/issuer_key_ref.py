"""Shared by the issuer-key tests: a Python restatement of IBM/idemix IssuerPublicKey.Check
(bccsp/schemes/dlog/crypto issuerkey.go) on the oracle curves, with the library's conventions,
and the mutations the tests run both through it and through the device.

    t1 = g2 s - W c,  t2 = BarG1 s - BarG2 c,
    c == HashToZr(t1 || t2 || g2 || BarG1 || W || BarG2)

G1 points are hashed as G1.Bytes(); G2 points as the four 32-byte coordinates of the ECP2 proto
in field order.  PINNED: the reference's four issuer keys (two per curve, tests/golden/idemix)
verify under this reading; tests/test_issuer_key_cpu.py shows that no other order of the four
coordinates verifies any of them."""
import os

from oracle import idemix as OI, idemix_identity as ID

import cred_issue_ref as R

OK, MALFORMED, UNDEFINED, PROOF = 0, 43, 44, 45
GOLDEN_KEYS = {"bn254": ("bn254_tokengen", "bn254_charlie"), "fp256bn": ("fp256bn_validator", "fp256bn_crypto")}
NAMES = (b"OU", b"Role", b"EnrollmentID", b"RevocationHandle")


def golden(issuer):
    with open(os.path.join(R.GOLD, issuer, "IssuerPublicKey"), "rb") as f:
        return f.read()


def g2_coords(PC, Q):
    """a G2 point (None: the identity) -> its four coordinates in the ECP2 proto's order"""
    if Q is None:  # gnark: zeros; AMCL: x = 0, y = 1
        return (0, 0, 0, 0) if PC is R.PR.BN254 else (0, 0, 1, 0)
    return tuple(int.from_bytes(v, "big") for _, _, v in OI.pb_fields(ID.ecp2(PC, Q)))


def g2_bytes(PC, Q, order=(0, 1, 2, 3)):
    c = g2_coords(PC, Q)
    return b"".join(c[k].to_bytes(32, "big") for k in order)


def fields(raw):
    """-> [(number, wire type, value)] of a well-formed key"""
    return OI.pb_fields(raw)


def rebuild(fs):
    """[(number, wire type, value bytes)] of length-delimited fields -> proto"""
    return b"".join(OI.pb_bytes_field(f, v) for f, _, v in fs)


def replace(raw, number, value, which=0):
    """the key with the `which`-th occurrence of field `number` set to `value` (None: removed)"""
    out, seen = [], 0
    for f, wt, v in fields(raw):
        if f == number:
            seen += 1
            if seen - 1 == which:
                if value is not None:
                    out.append((f, wt, value))
                continue
        out.append((f, wt, v))
    return rebuild(out)


def field(raw, number, which=0):
    return [v for f, _, v in fields(raw) if f == number][which]


def _g1(C, raw_ecp):
    """ECP proto -> a G1 point under the handles' rules; None: the identity (BN254: zeros)"""
    f = OI.pb_fields(raw_ecp)
    x, y = OI._pb_bytes(f, 1), OI._pb_bytes(f, 2)
    if len(x) != 32 or len(y) != 32:
        raise OI.PointError("ECP coordinate length")
    return C.g1_from_bytes(x + y if C is OI.BN254C else b"\x04" + x + y)


def _is_amcl_identity(raw_ecp):
    try:
        f = OI.pb_fields(raw_ecp)
        return OI._pb_bytes(f, 1) == bytes(32) and OI._pb_bytes(f, 2) == (1).to_bytes(32, "big")
    except ValueError:
        return False


def proof_parts(tag, raw):
    """-> a status other than OK, or (c, [t1, t2, g2, BarG1, W, BarG2]) of a key that reaches the
    proof, with the library's conventions and order of checks (include/fts_gpu.h)"""
    _, C, PC = R.CURVES[tag]
    if not raw:
        return MALFORMED
    try:
        fs = [(f, v) for f, wt, v in OI.pb_fields(raw) if wt == 2]
    except ValueError:
        return MALFORMED
    last = {f: v for f, v in fs}
    names, hattrs = [v for f, v in fs if f == 1], [v for f, v in fs if f == 4]
    if any(q not in last for q in (2, 3, 5, 6, 7, 8, 9)) or len(hattrs) < len(names):
        return UNDEFINED
    if len(last[8]) != 32 or len(last[9]) != 32:
        return MALFORMED
    try:
        for v in [last[2], last[3]] + hattrs:
            if _g1(C, v) is None:
                return MALFORMED
        if C is OI.FP256BNC and _is_amcl_identity(last[6]):
            return UNDEFINED
        bar1 = _g1(C, last[6])
        if bar1 is None:
            return UNDEFINED
        bar2 = _g1(C, last[7])
        w = ID.parse_ecp2(PC, last[5])
        if w is None:
            return MALFORMED
    except (ValueError, OI.PointError):
        return MALFORMED
    c, s = int.from_bytes(last[8], "big"), int.from_bytes(last[9], "big") % C.r
    if c >= C.r:  # Zr.Equals compares integers
        return PROOF
    t1 = PC.g2_add(PC.g2_mul(PC.g2_gen, s), PC.g2_neg(PC.g2_mul(w, c)))
    t2 = C.add(R.mul(C, bar1, s), C.neg(R.mul(C, bar2, c)))
    return c, [t1, t2, PC.g2_gen, bar1, w, bar2]


def challenge(tag, parts, order=(0, 1, 2, 3)):
    """HashToZr(t1 || t2 || g2 || BarG1 || W || BarG2); `order`: the order the four coordinates of
    a G2 point are hashed in"""
    _, C, PC = R.CURVES[tag]
    return C.hash_to_zr(b"".join(C.g1_bytes(pt) if k & 1 else g2_bytes(PC, pt, order) for k, pt in enumerate(parts)))


def check(tag, raw, order=(0, 1, 2, 3)):
    """IssuerPublicKey.Check -> OK, MALFORMED, UNDEFINED or PROOF"""
    p = proof_parts(tag, raw)
    if isinstance(p, int):
        return p
    return OK if challenge(tag, p[1], order) == p[0] else PROOF


def stored_hash(raw):
    return field(raw, 10)


def hash_of(tag, raw):
    _, C, _ = R.CURVES[tag]
    return OI.zr_bytes(C.hash_to_zr(OI.ipk_hash_input(raw)))


# ------------------------------------------------------------- mutations
def _zr_add(raw, number, delta):
    v = int.from_bytes(field(raw, number), "big") + delta
    return None if v >= 1 << 256 else replace(raw, number, v.to_bytes(32, "big"))


def _off_twist(PC, w_ecp2):
    """W with its last coordinate moved by one, until the point is off the twist"""
    f = [v for _, _, v in OI.pb_fields(w_ecp2)]
    for k in range(1, 8):
        g = list(f)
        g[3] = ((int.from_bytes(f[3], "big") + k) % PC.p).to_bytes(32, "big")
        cand = b"".join(OI.pb_bytes_field(i + 1, v) for i, v in enumerate(g))
        try:
            ID.parse_ecp2(PC, cand)
        except OI.PointError:
            return cand
    raise AssertionError("no off-twist neighbour")


def mutants(tag, raw):
    """-> [(name, key bytes or None, expected status)]: the honest key and the issue's mutations
    (ProofS + r and ProofC + r only where they fit 32 bytes)"""
    _, C, PC = R.CURVES[tag]
    w = ID.parse_ecp2(PC, field(raw, 5))
    bar1, bar2 = _g1(C, field(raw, 6)), _g1(C, field(raw, 7))
    ident = ID.ecp((0, 0)) if C is OI.BN254C else ID.ecp((0, 1))
    out = [("honest", raw, OK),
           ("proof_c+1", _zr_add(raw, 8, 1), PROOF),
           ("proof_s+1", _zr_add(raw, 9, 1), PROOF),
           ("proof_s+r", _zr_add(raw, 9, C.r), OK),
           ("proof_c+r", _zr_add(raw, 8, C.r), PROOF),
           ("w->2w", replace(raw, 5, ID.ecp2(PC, PC.g2_add(w, w))), PROOF),
           ("barg2->2barg2", replace(raw, 7, ID.ecp(C.add(bar2, bar2))), PROOF),
           ("barg1<->barg2", replace(replace(raw, 6, ID.ecp(bar2)), 7, ID.ecp(bar1)), PROOF),
           ("no barg1", replace(raw, 6, None), UNDEFINED),
           ("barg1 identity", replace(raw, 6, ident), UNDEFINED),
           # BarG2 is no base: gnark's identity decodes and its term vanishes; AMCL's is off the curve
           ("barg2 identity", replace(raw, 7, ident), PROOF if C is OI.BN254C else MALFORMED),
           ("no hrand", replace(raw, 3, None), UNDEFINED),
           ("one hattrs fewer", replace(raw, 4, None, which=1), UNDEFINED),
           ("31-byte proof_c", replace(raw, 8, field(raw, 8)[1:]), MALFORMED),
           ("w off the twist", replace(raw, 5, _off_twist(PC, field(raw, 5))), MALFORMED),
           ("truncated", raw[:len(raw) // 2 + 1], MALFORMED),
           ("empty", b"", MALFORMED)]
    return [m for m in out if m[1] is not None]


class ReplayRng:
    """a generator whose randrange returns the given values in order (make_issuer_key's draws)"""

    def __init__(self, values):
        self.values = list(values)
        self.used = 0

    def randrange(self, lo, hi=None):
        v = self.values[self.used]
        self.used += 1
        assert lo <= v < hi
        return v
