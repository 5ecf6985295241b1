"""Shared by the enrolment tests: a Python restatement of IBM/idemix NewCredRequest,
CredRequest.Check and NewCredential (bccsp/schemes/dlog/crypto credrequest.go, credential.go)
on the oracle curves, and make_issuer_key, which makes a complete IssuerPublicKey with its
secret on either curve (how FP256BN gets an issuer secret).

UNPINNED (no credential-request vector in the reference): the label "credRequest" and the
field order of the request transcript.  Pinned: the credential equation (Credential.Ver, which
the reference's signer configs pin) and bn254_tokengen/IssuerSecretKey, the reference's own.

The scalar products go through a Jacobian double-and-add written here (mul), a few
milliseconds each, so that a few hundred restated items stay within seconds;
tests/test_cred_issue_cpu.py checks it against the oracle curves' own mul."""
import os

from oracle import idemix as OI, idemix_identity as ID, pairing as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idemix")
LABEL = b"credRequest"
OK, BADKEY, MALFORMED, INVALID = 0, 34, 40, 41
# tag -> (mathlib CurveID, oracle curve, oracle pairing curve)
CURVES = {"bn254": (1, OI.BN254C, PR.BN254), "fp256bn": (0, OI.FP256BNC, PR.FP256BN)}
G1 = (1, 2)


def raw(issuer, name):
    with open(os.path.join(GOLD, issuer, name), "rb") as f:
        return f.read()


def tokengen():
    """-> (the reference's own BN254 issuer secret, its IssuerPublicKey proto)"""
    return int.from_bytes(raw("bn254_tokengen", "IssuerSecretKey"), "big"), raw("bn254_tokengen", "IssuerPublicKey")


# ------------------------------------------------------------- arithmetic
def mul(C, pt, k):
    """(k mod r) pt on y^2 = x^3 + 3, affine in and out (None: the identity)"""
    p = C.p
    k %= C.r
    if pt is None or k == 0:
        return None
    px, py = pt
    X, Y, Z = 0, 1, 0
    for bit in bin(k)[2:]:
        if Z:  # dbl-2009-l
            a, b = X * X % p, Y * Y % p
            c = b * b % p
            d = 2 * ((X + b) * (X + b) - a - c) % p
            e = 3 * a
            x3 = (e * e - 2 * d) % p
            Y, Z = (e * (d - x3) - 8 * c) % p, 2 * Y * Z % p
            X = x3
        if bit == "1":
            if not Z:
                X, Y, Z = px, py, 1
                continue
            z2 = Z * Z % p
            u2, s2 = px * z2 % p, py * z2 * Z % p
            h, r = (u2 - X) % p, (s2 - Y) % p
            assert h  # k < r and pt of order r: the running multiple is never +-pt here
            hh = h * h % p
            hhh, v = h * hh % p, X * hh % p
            x3 = (r * r - hhh - 2 * v) % p
            Y, Z = (r * (v - x3) - Y * hhh) % p, Z * h % p
            X = x3
    zi = pow(Z, -1, p)
    zi2 = zi * zi % p
    return (X * zi2 % p, Y * zi2 * zi % p)


def z32(v):
    return v.to_bytes(32, "big")


# ------------------------------------------------------------- the restatement
def _challenge(ipk, t, nym, nonce32):
    C = ipk["curve"]
    data = LABEL + C.g1_bytes(t) + C.g1_bytes(ipk["h_sk"]) + C.g1_bytes(nym) + nonce32 + \
        ipk["hash"][:32].ljust(32, b"\0")
    return C.hash_to_zr(data)


def encode_request(nym, nonce32, c, s):
    """CredRequest{1 nym: ECP{1 x, 2 y}, 2 issuer_nonce, 3 proof_c, 4 proof_s}; c, s: ints
    (written as Zr.Bytes()) or raw bytes"""
    b = lambda v: v if isinstance(v, bytes) else OI.zr_bytes(v)  # noqa: E731
    return OI.pb_bytes_field(1, ID.ecp(nym)) + OI.pb_bytes_field(2, nonce32) + OI.pb_bytes_field(3, b(c)) + \
        OI.pb_bytes_field(4, b(s))


def new_cred_request(ipk, sk, nonce32, r_sk):
    """NewCredRequest(sk, IssuerNonce, ipk) at the draw r_sk -> the proto"""
    C = ipk["curve"]
    nym, t = mul(C, ipk["h_sk"], sk), mul(C, ipk["h_sk"], r_sk)
    c = _challenge(ipk, t, nym, nonce32)
    return encode_request(nym, nonce32, c, (r_sk + c * sk) % C.r)


def _parse_request(ipk, req):
    """-> (Nym, nonce32, c, s) or None where the library says FTS_E_CREDREQ_MALFORMED"""
    C = ipk["curve"]
    if not req:
        return None
    try:
        f = OI.pb_fields(req)
        ecp, nonce, c, s = (OI._pb_bytes(f, k) for k in (1, 2, 3, 4))
        ef = OI.pb_fields(ecp)
        x, y = OI._pb_bytes(ef, 1), OI._pb_bytes(ef, 2)
    except ValueError:
        return None
    if any(len(v) != 32 for v in (nonce, c, s, x, y)):
        return None
    try:
        if C is OI.BN254C:
            nym = C.g1_from_bytes(x + y)
        else:
            nym = C.g1_from_bytes(b"\x04" + x + y)
    except OI.PointError:
        return None
    if nym is None:  # the identity (BN254: 64 zero bytes)
        return None
    return nym, nonce, int.from_bytes(c, "big"), int.from_bytes(s, "big")


def check_request(ipk, req):
    """CredRequest.Check(ipk) -> OK, MALFORMED or INVALID, with the library's conventions: proof_s
    is used mod r, a proof_c >= r can never equal the challenge"""
    C = ipk["curve"]
    p = _parse_request(ipk, req)
    if p is None:
        return MALFORMED
    nym, nonce, c, s = p
    if c >= C.r:
        return INVALID
    t = C.add(mul(C, ipk["h_sk"], s % C.r), C.neg(mul(C, nym, c)))
    return OK if c == _challenge(ipk, t, nym, nonce) else INVALID


def new_credential(ipk, isk, req, attrs, E, S):
    """NewCredential(isk, request, attrs) at the draws E, S, the request taken as checked ->
    the credential's parts (A, B, E, S, attrs)"""
    C = ipk["curve"]
    nym = _parse_request(ipk, req)[0]
    B = C.add(C.add(G1, nym), mul(C, ipk["h_rand"], S))
    for h, a in zip(ipk["h_attrs"], attrs):
        B = C.add(B, mul(C, h, a))
    return {"A": mul(C, B, pow((isk + E) % C.r, -1, C.r)), "B": B, "E": E, "S": S, "attrs": list(attrs)}


def cred_proto(k):
    """Credential{1 a, 2 b, 3 e, 4 s, 5 attrs}, the layout tests/cred_common.py cred_proto writes"""
    out = OI.pb_bytes_field(1, ID.ecp(k["A"])) + OI.pb_bytes_field(2, ID.ecp(k["B"])) + \
        OI.pb_bytes_field(3, OI.zr_bytes(k["E"])) + OI.pb_bytes_field(4, OI.zr_bytes(k["S"]))
    return out + b"".join(OI.pb_bytes_field(5, OI.zr_bytes(a)) for a in k["attrs"])


# ------------------------------------------------------------- a made issuer key
def make_issuer_key(tag, rng, isk=None):
    """-> (isk, IssuerPublicKey proto): HSk, HRand, HAttrs and BarG1 random multiples of g1,
    W = g2 isk, BarG2 = BarG1 isk, the proof of knowledge of isk (t1 = g2 r, t2 = BarG1 r,
    c = HashToZr(t1 || t2 || g2 || BarG1 || W || BarG2), s = r + c isk) and the hash over the
    proto without it.  On FP256BN the G2 points of the proof are hashed in the ECP2 proto's
    coordinate order; no fixture pins AMCL's G2 bytes, and nothing here checks that proof."""
    _, C, PC = CURVES[tag]
    isk = rng.randrange(1, C.r) if isk is None else isk
    pt = lambda: mul(C, G1, rng.randrange(1, C.r))  # noqa: E731
    h_sk, h_rand, h_attrs, bar_g1 = pt(), pt(), [pt() for _ in range(4)], pt()
    w, bar_g2 = PC.g2_mul(PC.g2_gen, isk), mul(C, bar_g1, isk)
    r = rng.randrange(1, C.r)
    t1, t2 = PC.g2_mul(PC.g2_gen, r), mul(C, bar_g1, r)
    if tag == "bn254":
        g2b = OI.g2_bytes
    else:
        g2b = lambda Q: b"".join(v for _, _, v in OI.pb_fields(ID.ecp2(PC, Q)))  # noqa: E731
    c = C.hash_to_zr(g2b(t1) + C.g1_bytes(t2) + g2b(PC.g2_gen) + C.g1_bytes(bar_g1) + g2b(w) + C.g1_bytes(bar_g2))
    s = (r + c * isk) % C.r
    out = b"".join(OI.pb_bytes_field(1, n) for n in (b"OU", b"Role", b"EnrollmentID", b"RevocationHandle"))
    out += OI.pb_bytes_field(2, ID.ecp(h_sk)) + OI.pb_bytes_field(3, ID.ecp(h_rand))
    out += b"".join(OI.pb_bytes_field(4, ID.ecp(h)) for h in h_attrs)
    out += OI.pb_bytes_field(5, ID.ecp2(PC, w)) + OI.pb_bytes_field(6, ID.ecp(bar_g1)) + \
        OI.pb_bytes_field(7, ID.ecp(bar_g2)) + OI.pb_bytes_field(8, OI.zr_bytes(c)) + OI.pb_bytes_field(9, OI.zr_bytes(s))
    return isk, out + OI.pb_bytes_field(10, OI.zr_bytes(C.hash_to_zr(out)))
