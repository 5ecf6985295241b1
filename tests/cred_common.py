"""Shared by the credential-verification tests: the reference's signer configs and issuer
keys (tests/golden/idemix), credentials issued with the oracle curve under the BN254 key whose
secret the fixtures hold, the Credential proto, and the rearranged pairing equation
e(W, A) e(g2, E A - B) = 1 on the oracle."""
import os

from oracle import idemix as OI, idemix_identity as ID, pairing as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idemix")
# issuer directory -> (mathlib CurveID, oracle curve, oracle pairing curve)
ISSUERS = {"bn254_charlie": (1, OI.BN254C, PR.BN254), "bn254_tokengen": (1, OI.BN254C, PR.BN254),
           "fp256bn_validator": (0, OI.FP256BNC, PR.FP256BN), "fp256bn_crypto": (0, OI.FP256BNC, PR.FP256BN)}


def raw(issuer, name):
    with open(os.path.join(GOLD, issuer, name), "rb") as f:
        return f.read()


def oracle_ipk(issuer):
    """-> (parsed issuer key, W)"""
    _, C, PC = ISSUERS[issuer]
    return OI.parse_ipk(raw(issuer, "IssuerPublicKey"), C), ID.ipk_w(PC, raw(issuer, "IssuerPublicKey"))


def signer(issuer, name="SignerConfig"):
    """a reference signer config -> the oracle's credential parts"""
    return ID.parse_signer_config(raw(issuer, name), ISSUERS[issuer][1])


def cred_proto(k, **over):
    """Credential{1 a, 2 b, 3 e, 4 s, 5 attrs} of the parts k, with fields replaced by `over`"""
    k = dict(k, **over)
    out = OI.pb_bytes_field(1, ID.ecp(k["A"])) + OI.pb_bytes_field(2, ID.ecp(k["B"])) + \
        OI.pb_bytes_field(3, OI.zr_bytes(k["E"])) + OI.pb_bytes_field(4, OI.zr_bytes(k["S"]))
    return out + b"".join(OI.pb_bytes_field(5, OI.zr_bytes(a)) for a in k["attrs"])


def issue_bn254(rng, E=None, plain_inverse=False):
    """a credential under bn254_tokengen, whose IssuerSecretKey the fixtures hold:
    B = credential_b(...), A = B (E + isk)^-1.  plain_inverse: A = B E^-1 instead, so that
    E A - B = O (not a valid credential: e(W, A) != 1)"""
    C = OI.BN254C
    ipk, _ = oracle_ipk("bn254_tokengen")
    isk = int.from_bytes(raw("bn254_tokengen", "IssuerSecretKey"), "big")
    k = {"E": rng.randrange(1, C.r) if E is None else E, "S": rng.randrange(C.r), "sk": rng.randrange(C.r),
         "attrs": [rng.randrange(C.r) for _ in range(4)]}
    k["B"] = ID.credential_b(ipk, k)
    k["A"] = C.mul(k["B"], pow(k["E"] if plain_inverse else (k["E"] + isk) % C.r, -1, C.r))
    return k


def rearranged_ok(issuer, W, k):
    """e(W, A) e(g2, E A - B) == 1"""
    _, C, PC = ISSUERS[issuer]
    T = C.add(C.mul(k["A"], k["E"]), C.neg(k["B"]))
    return PC.pairing_product_is_one([(W, k["A"]), (PC.g2_gen, T)])
