"""ECDSA P-256 owner signatures on the device (libfts_gpu.so
``fts_ecdsa_verify_batch``, ``fts_ecdsa_sign_batch``; include/fts_gpu.h).

Mirrors validator/ecdsa/ecdsa.go:69-113:

* ``Verifier(pk).Verify(message, sigma)`` raises ``SignatureError`` with the
  reference's message ("signature is not in lowS", "signature not valid", or
  the asn1 failure) — one item per device pass;
* ``verify_batch(items, device)`` is the batched form a validator uses for
  all owner signatures of many requests (TransferSignatureValidate,
  validator/validator_transfer.go:29-62, checks one per input).

Signing mirrors ecdsa.go:49-63: ``Signer(d).Sign(message)`` and the batched
``sign_batch(msgs, keys)`` return low-S DER signatures whose nonce is RFC 6979
(``mode="rfc6979"``) or RFC 6979 with per-item additional data (``"hedged"``, the
default), derived on the device; private keys are ints or 32 big-endian bytes.

Public keys are ``(x, y)`` ints, 64-byte X||Y, or the DER SubjectPublicKeyInfo
/ PEM "PUBLIC KEY" that ``Verifier.Serialize`` wraps (ecdsa.go:115-150).
There is no CPU fallback: every verdict comes from the HIP kernels.
"""
import base64
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import FTS_OK, FTS_E_SIG_MALFORMED, FTS_E_SIG_NOT_LOW_S, FTS_E_SIG_INVALID  # noqa: F401
from ._lib import FTS_E_SIGN_BADKEY, FTS_NONCE_RFC6979, FTS_NONCE_HEDGED  # noqa: F401
from ._lib import FTS_SEED_OS_RANDOM as OS_RANDOM

_MODES = {"rfc6979": FTS_NONCE_RFC6979, "hedged": FTS_NONCE_HEDGED}


class SignatureError(Exception):
    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status


def message(status):
    """Reference error string for a verdict (None for FTS_OK)."""
    if status == FTS_OK:
        return None
    if status == FTS_E_SIG_MALFORMED:
        return "asn1: structure error"
    return L.status_str(status)


def pk64_from_pkix(der):
    """x509.MarshalPKIXPublicKey bytes (or their PEM "PUBLIC KEY" block) -> X||Y."""
    if der.startswith(b"-----BEGIN"):
        lines = [ln for ln in der.decode().splitlines() if ln and not ln.startswith("-----")]
        der = base64.b64decode("".join(lines))
    out = (C.c_uint8 * 64)()
    L.check("fts_p256_pubkey_from_pkix", L.lib.fts_p256_pubkey_from_pkix(der, len(der), out))
    return bytes(out)


def _pk64(pk):
    if isinstance(pk, tuple):
        return pk[0].to_bytes(32, "big") + pk[1].to_bytes(32, "big")
    pk = bytes(pk)
    return pk if len(pk) == 64 else pk64_from_pkix(pk)


def parse_sig(sig):
    """Host-side asn1.Unmarshal + IsLowS + range checks -> (status, r, s)."""
    r, s, st = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), C.c_int32(0)
    L.check("fts_ecdsa_sig_parse", L.lib.fts_ecdsa_sig_parse(sig, len(sig), r, s, C.byref(st)))
    return st.value, int.from_bytes(bytes(r), "big"), int.from_bytes(bytes(s), "big")


def verify_batch(msgs, sigs, pks, device=0):
    """Verify n (message, DER signature, public key) triples in one device pass
    -> int32 status array."""
    n = len(msgs)
    if len(sigs) != n or len(pks) != n:
        raise ValueError("msgs, sigs and pks must have the same length")
    st = np.zeros(n, dtype=np.int32)
    if n == 0:
        return st
    keep = [(bytes(m), bytes(s), _pk64(p)) for m, s, p in zip(msgs, sigs, pks)]
    items = (L.EcdsaItem * n)()
    for i, (m, s, p) in enumerate(keep):
        items[i].msg = C.cast(C.c_char_p(m), C.c_void_p)
        items[i].msg_len = len(m)
        items[i].sig = C.cast(C.c_char_p(s), C.c_void_p)
        items[i].sig_len = len(s)
        items[i].pk64 = C.cast(C.c_char_p(p), C.c_void_p)
    L.check("fts_ecdsa_verify_batch",
            L.lib.fts_ecdsa_verify_batch(int(device), n, items, st.ctypes.data_as(C.POINTER(C.c_int32))))
    return st


def verify_packed(msg_buf, msg_off, msg_len, sig_buf, sig_off, sig_len, pk_buf, device=0):
    """Zero-copy batch form over contiguous buffers (bench / large batches).
    Every (offset, length) must lie inside its buffer and pk_buf must hold 64 bytes
    per item: the C library is handed raw pointers, so this is checked here
    (ValueError) before any pointer is formed."""
    n = len(msg_off)
    mo, ml = np.asarray(msg_off, dtype=np.uint64), np.asarray(msg_len, dtype=np.uint64)
    so, sl = np.asarray(sig_off, dtype=np.uint64), np.asarray(sig_len, dtype=np.uint64)
    if not (mo.shape == ml.shape == so.shape == sl.shape == (n,)):
        raise ValueError("offset and length arrays must be 1-D and of equal length")
    if len(pk_buf) < 64 * n:
        raise ValueError("pk_buf holds %d bytes, %d items need %d" % (len(pk_buf), n, 64 * n))
    for name, off, ln, buf in (("msg", mo, ml, msg_buf), ("sig", so, sl, sig_buf)):
        # end = off + len without uint64 wrap-around: off <= size and len <= size - off
        size = np.uint64(len(buf))
        if n and ((off > size).any() or (ln > size - np.minimum(off, size)).any()):
            raise ValueError("%s offset + length outside its buffer (%d bytes)" % (name, len(buf)))
    st = np.zeros(n, dtype=np.int32)
    items = np.zeros(n, dtype=[("msg", "u8"), ("msg_len", "u8"), ("sig", "u8"), ("sig_len", "u8"), ("pk64", "u8")])
    mb, sb, pb = (np.frombuffer(b, dtype=np.uint8) for b in (msg_buf, sig_buf, pk_buf))
    items["msg"] = mb.ctypes.data + mo
    items["msg_len"] = ml
    items["sig"] = sb.ctypes.data + so
    items["sig_len"] = sl
    items["pk64"] = pb.ctypes.data + 64 * np.arange(n, dtype=np.uint64)
    L.check("fts_ecdsa_verify_batch",
            L.lib.fts_ecdsa_verify_batch(int(device), n, items.ctypes.data_as(C.POINTER(L.EcdsaItem)),
                                         st.ctypes.data_as(C.POINTER(C.c_int32))))
    return st


def last_timings(device=0):
    """{kernel: ms} of the last verify call on `device` (HIP events)."""
    ms = (C.c_float * 2)()
    L.check("fts_ecdsa_last_timings", L.lib.fts_ecdsa_last_timings(int(device), ms))
    return {"k_ecdsa_digest": ms[0], "k_ecdsa_verify": ms[1]}


def _d32(d):
    if isinstance(d, int):
        # out-of-range ints still reach the library, which rejects them per item
        return (d & ((1 << 256) - 1)).to_bytes(32, "big") if 0 <= d < (1 << 256) else b"\xff" * 32
    d = bytes(d)
    if len(d) != 32:
        raise ValueError("a private key is an int or 32 big-endian bytes")
    return d


def sig_encode(r, s):
    """utils.MarshalECDSASignature(r, s): minimal DER (host only)."""
    out, n = (C.c_uint8 * L.FTS_ECDSA_SIG_MAX)(), C.c_uint32(0)
    L.check("fts_ecdsa_sig_encode",
            L.lib.fts_ecdsa_sig_encode(r.to_bytes(32, "big"), s.to_bytes(32, "big"), out, C.byref(n)))
    return bytes(out[:n.value])


def sign_batch(msgs, keys, device=0, mode="hedged", seed=OS_RANDOM, return_status=False):
    """Sign msgs[i] under keys[i] in one device pass -> list of DER signatures
    (``b""`` for a key outside [1, n-1]; with ``return_status`` also the int32 statuses).
    mode: "hedged" (RFC 6979 section 3.6, additional data from `seed`; OS_RANDOM = the
    secure source) or "rfc6979" (deterministic, `seed` ignored)."""
    n = len(msgs)
    if len(keys) != n:
        raise ValueError("msgs and keys must have the same length")
    if mode not in _MODES:
        raise ValueError("mode is 'hedged' or 'rfc6979'")
    st = np.zeros(n, dtype=np.int32)
    if n == 0:
        return ([], st) if return_status else []
    keep = [(bytes(m), _d32(d)) for m, d in zip(msgs, keys)]
    items = (L.EcdsaSignItem * n)()
    for i, (m, d) in enumerate(keep):
        items[i].msg = C.cast(C.c_char_p(m), C.c_void_p)
        items[i].msg_len = len(m)
        items[i].d32 = C.cast(C.c_char_p(d), C.c_void_p)
    sig = np.zeros(n * L.FTS_ECDSA_SIG_MAX, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint32)
    L.check("fts_ecdsa_sign_batch",
            L.lib.fts_ecdsa_sign_batch(int(device), n, items, _MODES[mode], int(seed) & ((1 << 64) - 1),
                                       sig.ctypes.data, ln.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       st.ctypes.data_as(C.POINTER(C.c_int32))))
    raw = sig.tobytes()
    out = [raw[i * L.FTS_ECDSA_SIG_MAX:i * L.FTS_ECDSA_SIG_MAX + int(ln[i])] for i in range(n)]
    return (out, st) if return_status else out


def sign_last_timings(device=0):
    """{kernel: ms} of the last signing call on `device` (HIP events)."""
    ms = (C.c_float * 2)()
    L.check("fts_ecdsa_sign_last_timings", L.lib.fts_ecdsa_sign_last_timings(int(device), ms))
    return {"k_ecdsa_digest": ms[0], "k_ecdsa_sign": ms[1]}


class Signer:
    """ecdsa.Signer{SK} (validator/ecdsa/ecdsa.go:38-63): Sign returns the low-S DER
    signature of SHA-256(message)."""

    def __init__(self, d, device=0, mode="hedged", seed=OS_RANDOM):
        self.d32 = _d32(d)
        self.device, self.mode, self.seed = device, mode, seed

    def Sign(self, message_):
        sigs, st = sign_batch([message_], [self.d32], self.device, self.mode, self.seed, return_status=True)
        if int(st[0]) != FTS_OK:
            raise SignatureError(message(int(st[0])), int(st[0]))
        return sigs[0]


class Verifier:
    """ecdsa.Verifier{PK} (validator/ecdsa/ecdsa.go:69-113)."""

    def __init__(self, pk, device=0):
        self.pk64 = _pk64(pk)
        self.device = device

    def Verify(self, message_, sigma):
        st = int(verify_batch([message_], [sigma], [self.pk64], self.device)[0])
        if st != FTS_OK:
            raise SignatureError(message(st), st)
