"""RFC 6979 (deterministic ECDSA nonces, HMAC-DRBG over SHA-256) for P-256, written
with hmac / hashlib only: the reference the signing tests compare the library's
nonce derivation with.  `extra` is the additional data of section 3.6."""
import hashlib
import hmac

from oracle import ecdsa_p256 as E

N = E.N
RFC_KEY = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721


def _mac(key, data):
    return hmac.new(key, data, hashlib.sha256).digest()


def candidates(d, h1, extra=b""):
    """the candidate stream of section 3.2 step h for private key d and digest h1
    (32 bytes): every in-range k in order, as if each one were then rejected"""
    x = d.to_bytes(32, "big")
    hr = (int.from_bytes(h1, "big") % N).to_bytes(32, "big")  # bits2octets (qlen = hlen)
    v, k = b"\x01" * 32, b"\x00" * 32
    k = _mac(k, v + b"\x00" + x + hr + extra)
    v = _mac(k, v)
    k = _mac(k, v + b"\x01" + x + hr + extra)
    v = _mac(k, v)
    while True:
        v = _mac(k, v)
        c = int.from_bytes(v, "big")
        if 1 <= c < N:
            yield c
        k = _mac(k, v + b"\x00")
        v = _mac(k, v)


def nonce(d, msg, extra=b""):
    return next(candidates(d, hashlib.sha256(msg).digest(), extra))


def raw_s(d, msg, k):
    """s before the low-S rule"""
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big")
    r = E.mul(k, E.G)[0] % N
    return pow(k, -1, N) * (e + r * d) % N
