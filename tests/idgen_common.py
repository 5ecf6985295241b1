"""Shared by the identity-generation tests: the reference's credentials (tests/golden/idemix),
the oracle's signer driven with given draws, and the values an identity is written from."""
import os

from oracle import idemix as OI, idemix_identity as ID, pairing as PR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# tag -> (fixture directory, mathlib CurveID, oracle curve, oracle pairing curve)
CURVES = {"bn254": ("bn254_charlie", 1, OI.BN254C, PR.BN254),
          "fp256bn": ("fp256bn_validator", 0, OI.FP256BNC, PR.FP256BN)}


def raw(tag, name):
    with open(os.path.join(GOLD, "idemix", CURVES[tag][0], name), "rb") as f:
        return f.read()


def oracle_key(tag):
    """-> (parsed issuer key, parsed credential, W)"""
    _, _, C, PC = CURVES[tag]
    return OI.parse_ipk(raw(tag, "IssuerPublicKey"), C), ID.parse_signer_config(raw(tag, "SignerConfig"), C), \
        ID.ipk_w(PC, raw(tag, "IssuerPublicKey"))


class Stub:
    """stands in for random.Random in the oracle's sign: hands out the given values in order"""

    def __init__(self, vals):
        self.vals = list(vals)

    def randrange(self, *_):
        return self.vals.pop(0)


def oracle_sign(tag, ipk, cred, draws, epoch=0):
    """the oracle's signature dict and Nym at the library's 18 draws (rnym first)"""
    stub = Stub(draws[1:])
    sig, nym = ID.sign(ipk, cred, draws[0], stub, CURVES[tag][3], epoch=epoch)
    assert not stub.vals
    return sig, nym


def oracle_identity(tag, ipk, cred, draws, epoch=0):
    C, PC = CURVES[tag][2], CURVES[tag][3]
    sig, nym = oracle_sign(tag, ipk, cred, draws, epoch)
    return ID.serialize_identity(C.g1_bytes(nym), ID.encode_signature(sig, PC))


def writer_inputs(sig):
    """a signature dict -> (points, scalars, nonce) in the identity writer's order"""
    pts = [sig[k] for k in ("APrime", "ABar", "BPrime", "Nym", "EidNym", "RhNym")]
    sc = [sig[k] for k in ("c", "sSk", "sE", "sR2", "sR3", "sSPrime")] + list(sig["sAttrs"]) + \
        [sig["sRNym"], sig["sEid"], sig["sRh"]]
    return pts, sc, sig["nonce"]
