"""Idemix pseudonym (nym) signatures on the device (libfts_gpu.so
``fts_nym_verify_batch``; include/fts_gpu.h).

Mirrors services/identity/idemix/crypto/id.go:145-161:

* ``NymSignatureVerifier(ipk, nym_pk).Verify(message, sigma)`` raises
  ``SignatureError`` with the reference's message;
* ``IssuerKey(ipk_bytes).verify_batch(nyms, sigs, msgs)`` is the batched form
  a validator uses for the owner signatures of idemix-owned inputs
  (TransferSignatureValidate, validator/validator_transfer.go:29-62).

Signing: ``IssuerKey.sign_batch(sks, rnyms, nyms, msgs)`` and
``NymSigner(issuer_key, sk, rnym, nym).Sign(message)`` produce the NymSignature
protos that the verifiers above accept (k_nym_sign<BnCurve> / k_nym_sign<FbnCurve>).

Identities: ``IdentityVerifier`` checks owner identities and matches audit info against
them; ``Credential(verifier, cred, sk).generate(n)`` produces them on the device
(KeyManager.Identity, services/identity/idemix/km.go:173-290);
``IdentityVerifier.verify_credentials(creds, sks)`` / ``VerifyCredential(cred, sk)`` check
credentials as NewKeyManager does, pairing equation included (km.go:117-133).

Enrolment: ``IdentityVerifier.make_cred_requests(sks, nonces)`` is the wallet's
NewCredRequest, ``IdentityVerifier.verify_cred_requests(reqs)`` CredRequest.Check, and
``Issuer(verifier, isk).issue(reqs, attrs)`` checks each request and issues its credential
(NewCredential), so that request -> credential -> ``Credential`` -> identities -> verified
identities runs on the device end to end.

Issuer keys: ``check_issuer_keys(ipks, curve)`` is IssuerPublicKey.Check (the key's proof of
knowledge of its secret, G2 side included) and ``generate_issuer_keys(n, curve)`` NewIssuerKey,
so the chain above can start from a key made on the device.

The issuer key is the idemix IssuerPublicKey proto a zkatdlog PublicParams
carries, on BN254 (the tokengen key of zkatdlog_pp.json) or FP256BN_AMCL (the
validator's test keys).  There is no CPU fallback: every verdict comes from
the HIP kernels k_nym_verify (BN254, idemix_kernels.hip) and k_nym_verify<FbnCurve> (device/nym_kernels.hpp).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import FTS_OK, FTS_E_NYM_MALFORMED, FTS_E_NYM_BADKEY, FTS_E_NYM_INVALID  # noqa: F401
from ._lib import (FTS_E_ID_MALFORMED, FTS_E_ID_BADNYM, FTS_E_ID_NO_EIDNYM, FTS_E_ID_NO_RHNYM,  # noqa: F401
                   FTS_E_ID_REVOCATION, FTS_E_ID_APRIME, FTS_E_ID_PAIRING, FTS_E_ID_ZK)
from ._lib import (FTS_E_AUDIT_MALFORMED, FTS_E_AUDIT_NO_EIDNYM, FTS_E_AUDIT_EID_POINT,  # noqa: F401
                   FTS_E_AUDIT_EID_MISMATCH, FTS_E_AUDIT_NO_RHNYM, FTS_E_AUDIT_RH_POINT, FTS_E_AUDIT_RH_MISMATCH)
from ._lib import FTS_CURVE_BN254, FTS_CURVE_FP256BN_AMCL  # noqa: F401
from ._lib import FTS_E_SIGN_BADKEY, FTS_NYM_SIG_LEN  # noqa: F401
from ._lib import FTS_E_CRED_MALFORMED, FTS_E_CRED_B, FTS_E_CRED_PAIRING  # noqa: F401
from ._lib import FTS_E_CREDREQ_MALFORMED, FTS_E_CREDREQ_INVALID  # noqa: F401
from ._lib import FTS_IDEMIX_CRED_REQUEST_LEN, FTS_IDEMIX_CREDENTIAL_LEN  # noqa: F401
from ._lib import FTS_E_IPK_MALFORMED, FTS_E_IPK_UNDEFINED, FTS_E_IPK_PROOF, FTS_IDEMIX_IPK_LEN  # noqa: F401
from ._lib import FTS_SEED_OS_RANDOM as OS_RANDOM


class SignatureError(Exception):
    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status


def message(status):
    """Reference error string for a verdict (None for FTS_OK)."""
    return None if status == FTS_OK else L.status_str(status)


def identity_nym(serialized_identity):
    """SerializedIdemixIdentity.nym_public_key (crypto/deserializer.go:41-56)."""
    raw = bytes(serialized_identity)
    p, n = C.c_void_p(), C.c_size_t()
    L.check("fts_idemix_identity_nym", L.lib.fts_idemix_identity_nym(raw, len(raw), C.byref(p), C.byref(n)))
    off = p.value - C.cast(C.c_char_p(raw), C.c_void_p).value
    return raw[off:off + n.value]


class IssuerKey:
    """Device-resident idemix issuer public key (HSk / HRand fixed-base tables)."""

    def __init__(self, ipk, device=0, curve=FTS_CURVE_BN254):
        """curve: mathlib CurveID (PublicParams.IdemixIssuerPublicKeys[i].Curve)."""
        self.ipk = bytes(ipk)
        self.device = device
        self.curve = curve
        self.nym_len = 64 if curve == FTS_CURVE_BN254 else 65
        h = C.c_void_p()
        L.check("fts_idemix_ipk_create",
                L.lib.fts_idemix_ipk_create(int(device), self.ipk, len(self.ipk), int(curve), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            L.lib.fts_idemix_ipk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_batch(self, nyms, sigs, msgs):
        """n (nym public key, NymSignature, message) triples in one device pass
        -> int32 status array."""
        n = len(nyms)
        if len(sigs) != n or len(msgs) != n:
            raise ValueError("nyms, sigs and msgs must have the same length")
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return st
        keep = [(bytes(a), bytes(b), bytes(c)) for a, b, c in zip(nyms, sigs, msgs)]
        items = (L.NymItem * n)()
        for i, (a, b, c) in enumerate(keep):
            items[i].nym = C.cast(C.c_char_p(a), C.c_void_p)
            items[i].nym_len = len(a)
            items[i].sig = C.cast(C.c_char_p(b), C.c_void_p)
            items[i].sig_len = len(b)
            items[i].msg = C.cast(C.c_char_p(c), C.c_void_p)
            items[i].msg_len = len(c)
        L.check("fts_nym_verify_batch",
                L.lib.fts_nym_verify_batch(self.h, n, items, st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def verify_packed(self, nym_buf, sig_buf, sig_off, sig_len, msg_buf, msg_off, msg_len):
        """Zero-copy batch over contiguous buffers (nym keys of self.nym_len bytes back to back);
        bounds are checked here before any raw pointer is formed."""
        n = len(sig_off)
        so, sl = np.asarray(sig_off, dtype=np.uint64), np.asarray(sig_len, dtype=np.uint64)
        mo, ml = np.asarray(msg_off, dtype=np.uint64), np.asarray(msg_len, dtype=np.uint64)
        if not (so.shape == sl.shape == mo.shape == ml.shape == (n,)):
            raise ValueError("offset and length arrays must be 1-D and of equal length")
        nl = self.nym_len
        if len(nym_buf) < nl * n:
            raise ValueError("nym_buf holds %d bytes, %d items need %d" % (len(nym_buf), n, nl * n))
        for name, off, ln, buf in (("sig", so, sl, sig_buf), ("msg", mo, ml, msg_buf)):
            size = np.uint64(len(buf))
            if n and ((off > size).any() or (ln > size - np.minimum(off, size)).any()):
                raise ValueError("%s offset + length outside its buffer (%d bytes)" % (name, len(buf)))
        st = np.zeros(n, dtype=np.int32)
        items = np.zeros(n, dtype=[("nym", "u8"), ("nym_len", "u8"), ("sig", "u8"), ("sig_len", "u8"),
                                   ("msg", "u8"), ("msg_len", "u8")])
        nb, sb, mb = (np.frombuffer(b, dtype=np.uint8) for b in (nym_buf, sig_buf, msg_buf))
        items["nym"] = nb.ctypes.data + nl * np.arange(n, dtype=np.uint64)
        items["nym_len"] = nl
        items["sig"] = sb.ctypes.data + so
        items["sig_len"] = sl
        items["msg"] = mb.ctypes.data + mo
        items["msg_len"] = ml
        L.check("fts_nym_verify_batch",
                L.lib.fts_nym_verify_batch(self.h, n, items.ctypes.data_as(C.POINTER(L.NymItem)),
                                           st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def last_kernel_ms(self):
        ms = C.c_float()
        L.check("fts_nym_last_timings", L.lib.fts_nym_last_timings(self.h, C.byref(ms)))
        return ms.value

    def sign_batch(self, sks, rnyms, nyms, msgs, seed=OS_RANDOM, return_status=False):
        """n nym signatures in one device pass -> list of 136-byte NymSignature protos
        (``b""`` for a rejected item; with ``return_status`` also the int32 statuses).
        sks / rnyms: ints or 32 big-endian bytes below the curve's r; nyms: G1.Bytes() of
        Nym = HSk^sk HRand^rnym.  seed: OS_RANDOM = the secure source, else test-only."""
        n = len(msgs)
        if not (len(sks) == len(rnyms) == len(nyms) == n):
            raise ValueError("sks, rnyms, nyms and msgs must have the same length")
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return ([], st) if return_status else []

        def z32(v):
            if isinstance(v, int):
                return v.to_bytes(32, "big") if 0 <= v < (1 << 256) else b"\xff" * 32
            v = bytes(v)
            if len(v) != 32:
                raise ValueError("a secret is an int or 32 big-endian bytes")
            return v
        keep = [(z32(a), z32(b), bytes(c), bytes(d)) for a, b, c, d in zip(sks, rnyms, nyms, msgs)]
        items = (L.NymSignItem * n)()
        for i, (a, b, c, d) in enumerate(keep):
            items[i].sk32 = C.cast(C.c_char_p(a), C.c_void_p)
            items[i].rnym32 = C.cast(C.c_char_p(b), C.c_void_p)
            items[i].nym = C.cast(C.c_char_p(c), C.c_void_p)
            items[i].nym_len = len(c)
            items[i].msg = C.cast(C.c_char_p(d), C.c_void_p)
            items[i].msg_len = len(d)
        sig = np.zeros(n * FTS_NYM_SIG_LEN, dtype=np.uint8)
        L.check("fts_nym_sign_batch",
                L.lib.fts_nym_sign_batch(self.h, n, items, int(seed) & ((1 << 64) - 1), sig.ctypes.data,
                                         st.ctypes.data_as(C.POINTER(C.c_int32))))
        raw = sig.tobytes()
        out = [raw[i * FTS_NYM_SIG_LEN:(i + 1) * FTS_NYM_SIG_LEN] if st[i] == FTS_OK else b"" for i in range(n)]
        return (out, st) if return_status else out

    def last_sign_kernel_ms(self):
        ms = C.c_float()
        L.check("fts_nym_sign_last_timings", L.lib.fts_nym_sign_last_timings(self.h, C.byref(ms)))
        return ms.value


class NymSigner:
    """The nym signer of services/identity/idemix/crypto/id.go: Sign returns the
    NymSignature proto over `message` for the pseudonym (sk, rnym, nym)."""

    def __init__(self, issuer_key, sk, rnym, nym_pk, seed=OS_RANDOM):
        self.ipk, self.sk, self.rnym, self.nym, self.seed = issuer_key, sk, rnym, bytes(nym_pk), seed

    def Sign(self, message_):
        sigs, st = self.ipk.sign_batch([self.sk], [self.rnym], [self.nym], [message_], self.seed, return_status=True)
        if int(st[0]) != FTS_OK:
            raise SignatureError(message(int(st[0])), int(st[0]))
        return sigs[0]


class NymSignatureVerifier:
    """crypto.NymSignatureVerifier{IPK, NymPK} (id.go:145-161)."""

    def __init__(self, issuer_key, nym_pk):
        self.ipk = issuer_key
        self.nym = bytes(nym_pk)

    def Verify(self, message_, sigma):
        st = int(self.ipk.verify_batch([self.nym], [sigma], [message_])[0])
        if st != FTS_OK:
            raise SignatureError(message(st), st)


class IdentityVerifier:
    """Idemix identity validity on the device (fts_idemix_identity_verify_batch):
    the check ``Deserializer.Deserialize(raw, true)`` makes for every idemix owner
    (services/identity/idemix/deserializer.go:82-93 -> crypto/id.go:74-108, IBM/idemix
    Signature.Ver with ExpectEidNymRhNym).  One handle per issuer public key."""

    def __init__(self, ipk, device=0, curve=FTS_CURVE_BN254):
        self.ipk = bytes(ipk)
        self.device = device
        self.curve = curve
        h = C.c_void_p()
        L.check("fts_idemix_idv_create",
                L.lib.fts_idemix_idv_create(int(device), self.ipk, len(self.ipk), int(curve), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            L.lib.fts_idemix_idv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, identities):
        """the C-ABI's pointer / length arrays for a batch of serialized identities,
        built once: verify_prepared then calls the library with no per-call Python
        marshaling (a Go caller hands its slices' pointers over the same way)"""
        keep = [bytes(x) for x in identities]
        n = len(keep)
        ptrs = (C.c_void_p * max(1, n))(*[C.cast(C.c_char_p(b), C.c_void_p).value for b in keep])
        lens = (C.c_size_t * max(1, n))(*[len(b) for b in keep])
        return keep, ptrs, lens

    def verify_prepared(self, prep):
        """prepare()d identities -> int32 status array (FTS_OK or FTS_E_ID_*)"""
        keep, ptrs, lens = prep
        n = len(keep)
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return st
        L.check("fts_idemix_identity_verify_batch",
                L.lib.fts_idemix_identity_verify_batch(self.h, n, ptrs, lens, st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def verify_batch(self, identities):
        """serialized identities -> int32 status array (FTS_OK or FTS_E_ID_*)"""
        return self.verify_prepared(self.prepare(identities))

    def Deserialize(self, identity):
        """raises IdentityError with the reference's message, as Deserialize(raw, true) errors"""
        st = int(self.verify_batch([identity])[0])
        if st != FTS_OK:
            raise IdentityError(message(st), st)

    def last_kernel_ms(self):
        """(decode + t-values + transcript, pairings) HIP-event ms of the last batch"""
        ms = (C.c_float * 2)()
        L.check("fts_idemix_identity_last_timings", L.lib.fts_idemix_identity_last_timings(self.h, ms))
        return float(ms[0]), float(ms[1])

    def last_pairing_stats(self):
        """(groups checked with one randomised pairing product, identities paired one by
        one) of the last batch; (0, n) with FTS_IDV_BATCH=0"""
        out = (C.c_uint32 * 2)()
        L.check("fts_idemix_identity_last_stats", L.lib.fts_idemix_identity_last_stats(self.h, out))
        return int(out[0]), int(out[1])

    def audit_match_batch(self, identities, eids=(), r_eids=(), rhs=(), r_rhs=()):
        """AuditInfo.Match (services/identity/idemix/crypto/audit.go:40-84) for n owner
        identities in one device pass (fts_idemix_audit_match_batch): eids / rhs are
        AuditInfo.Attributes[2] / [3], r_eids / r_rhs the 32-byte Rand.Bytes() of
        EidNymAuditData / RhNymAuditData (None: a nil Rand).  The identity's proof is
        not verified here (verify_batch).  -> int32 status array (FTS_OK or FTS_E_AUDIT_*)"""
        n = len(identities)
        if not (len(eids) == len(r_eids) == len(rhs) == len(r_rhs) == n):
            raise ValueError("identities, eids, r_eids, rhs and r_rhs must have the same length")
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return st
        for r in list(r_eids) + list(r_rhs):
            if r is not None and len(r) != 32:
                raise ValueError("a rand is 32 bytes (Zr.Bytes())")

        def ptr(b):  # None: NULL; b"" keeps a valid pointer
            return None if b is None else C.cast(C.c_char_p(b), C.c_void_p)
        keep = [tuple(None if x is None else bytes(x) for x in t) for t in zip(identities, eids, r_eids, rhs, r_rhs)]
        items = (L.AuditItem * n)()
        for i, (ident, eid, r_eid, rh, r_rh) in enumerate(keep):
            it = items[i]
            it.id, it.id_len = ptr(ident), len(ident or b"")
            it.eid, it.eid_len = ptr(eid), len(eid or b"")
            it.rh, it.rh_len = ptr(rh), len(rh or b"")
            it.r_eid32, it.r_rh32 = ptr(r_eid), ptr(r_rh)
        L.check("fts_idemix_audit_match_batch",
                L.lib.fts_idemix_audit_match_batch(self.h, n, items, st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def Match(self, identity, eid, r_eid, rh, r_rh):
        """raises AuditMatchError with the reference's message, as AuditInfo.Match errors"""
        st = int(self.audit_match_batch([identity], [eid], [r_eid], [rh], [r_rh])[0])
        if st != FTS_OK:
            raise AuditMatchError(message(st), st)

    def last_audit_kernel_ms(self):
        """HIP-event ms of the last audit_match_batch's kernel"""
        ms = C.c_float()
        L.check("fts_idemix_audit_last_timings", L.lib.fts_idemix_audit_last_timings(self.h, C.byref(ms)))
        return ms.value

    def verify_credentials(self, creds, sks):
        """Credential.Ver under the handle's issuer key, pairing equation included, for n
        (Credential proto, user secret) pairs in one device pass (fts_idemix_cred_verify_batch;
        services/identity/idemix/km.go:117-133).  sks: ints or 32 big-endian bytes; None for
        either input is a NULL pointer.  -> int32 status array (FTS_OK or FTS_E_CRED_*)"""
        n = len(creds)
        if len(sks) != n:
            raise ValueError("creds and sks must have the same length")
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return st

        def z32(v):
            if v is None:
                return None
            if isinstance(v, int):
                return v.to_bytes(32, "big") if 0 <= v < (1 << 256) else b"\xff" * 32
            v = bytes(v)
            if len(v) != 32:
                raise ValueError("the user secret is an int or 32 big-endian bytes")
            return v

        def ptr(b):  # None: NULL; b"" keeps a valid pointer
            return None if b is None else C.cast(C.c_char_p(b), C.c_void_p)
        keep = [(None if c is None else bytes(c), z32(s)) for c, s in zip(creds, sks)]
        items = (L.CredItem * n)()
        for i, (c, s) in enumerate(keep):
            items[i].cred, items[i].cred_len, items[i].sk32 = ptr(c), len(c or b""), ptr(s)
        L.check("fts_idemix_cred_verify_batch",
                L.lib.fts_idemix_cred_verify_batch(self.h, n, items, st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def VerifyCredential(self, cred, sk):
        """raises IdentityError with the reference's message, as NewKeyManager does for a
        signer config whose credential does not verify"""
        st = int(self.verify_credentials([cred], [sk])[0])
        if st != FTS_OK:
            raise IdentityError(message(st), st)

    def last_cred_kernel_ms(self):
        """(decode + products + B check, pairing stage) HIP-event ms of the last credential batch"""
        ms = (C.c_float * 2)()
        L.check("fts_idemix_cred_verify_last_timings", L.lib.fts_idemix_cred_verify_last_timings(self.h, ms))
        return float(ms[0]), float(ms[1])

    def last_cred_stats(self):
        """(groups checked with one randomised pairing product, credentials paired one by
        one) of the last credential batch; (0, n) with FTS_IDV_BATCH=0"""
        out = (C.c_uint32 * 2)()
        L.check("fts_idemix_cred_verify_last_stats", L.lib.fts_idemix_cred_verify_last_stats(self.h, out))
        return int(out[0]), int(out[1])

    def make_cred_requests(self, sks, nonces, seed=None, stride=None):
        """NewCredRequest for n (user secret, issuer nonce) pairs in one device pass
        (fts_idemix_cred_request_batch).  sks, nonces: ints or 32 big-endian bytes; seed None:
        the secure source, else test-only (item i equals the one-item call at seed + i).
        -> (requests: CredRequest protos, b"" for a rejected item; int32 status array)"""
        n = len(sks)
        if len(nonces) != n:
            raise ValueError("sks and nonces must have the same length")
        ln = FTS_IDEMIX_CRED_REQUEST_LEN
        stride = ln if stride is None else int(stride)
        st = np.zeros(n, dtype=np.int32)
        skb = np.frombuffer(b"".join(_z32(v) for v in sks) or b"\0", dtype=np.uint8)
        nb = np.frombuffer(b"".join(_z32(v) for v in nonces) or b"\0", dtype=np.uint8)
        out = np.zeros(max(1, n * stride), dtype=np.uint8)
        lens = np.zeros(max(1, n), dtype=np.uint32)
        sd = OS_RANDOM if seed is None else int(seed) & ((1 << 64) - 1)
        L.check("fts_idemix_cred_request_batch",
                L.lib.fts_idemix_cred_request_batch(self.h, n, skb.ctypes.data, nb.ctypes.data, sd, out.ctypes.data,
                                                    stride, lens.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_int32))))
        raw = out.tobytes()
        self.last_request_buffer = raw[:n * stride]  # rejected items: zeros
        return [raw[i * stride:i * stride + int(lens[i])] for i in range(n)], st

    def verify_cred_requests(self, reqs):
        """CredRequest.Check for n requests in one device pass (fts_idemix_cred_request_verify_batch;
        None is a NULL pointer) -> int32 status array (FTS_OK or FTS_E_CREDREQ_*)"""
        n = len(reqs)
        st = np.zeros(n, dtype=np.int32)
        if n == 0:
            return st
        keep = [None if r is None else bytes(r) for r in reqs]
        items = (L.CredReqItem * n)()
        for i, r in enumerate(keep):
            items[i].req = None if r is None else C.cast(C.c_char_p(r), C.c_void_p)
            items[i].req_len = len(r or b"")
        L.check("fts_idemix_cred_request_verify_batch",
                L.lib.fts_idemix_cred_request_verify_batch(self.h, n, items, st.ctypes.data_as(C.POINTER(C.c_int32))))
        return st

    def last_cred_request_kernel_ms(self):
        """HIP-event ms of (the last make_cred_requests, the last verify_cred_requests)"""
        ms = (C.c_float * 2)()
        L.check("fts_idemix_cred_request_last_timings", L.lib.fts_idemix_cred_request_last_timings(self.h, ms))
        return float(ms[0]), float(ms[1])

    def pairing_debug(self, which, p64, final_exp=True):
        """e(W or g2, P) on the handle's curve, P = X || Y (64 raw BE bytes): 6 Fp2
        coefficients (w^0..w^5) as Montgomery ints"""
        out = (C.c_uint32 * 192)()
        L.check("fts_idemix_pairing_debug",
                L.lib.fts_idemix_pairing_debug(self.h, int(which), bytes(p64), int(bool(final_exp)), out))
        w = list(out)
        val = lambda o: sum(w[o + i] << (32 * i) for i in range(8))  # noqa: E731
        return [(val(16 * k), val(16 * k + 8)) for k in range(6)]


def _z32(v):
    """an int or 32 big-endian bytes -> 32 bytes (an int outside [0, 2^256): all ones, which is
    above either r)"""
    if isinstance(v, int):
        return v.to_bytes(32, "big") if 0 <= v < (1 << 256) else b"\xff" * 32
    v = bytes(v)
    if len(v) != 32:
        raise ValueError("a scalar is an int or 32 big-endian bytes")
    return v


class Issuer:
    """One idemix issuer secret on the device (fts_idemix_issuer): issue(reqs, attrs) is what n
    calls of CredRequest.Check and NewCredential do.  Borrows `verifier` (an IdentityVerifier
    under the issuer's public key), which must stay open while this handle lives.  Raises
    FtsError (FTS_API_EPP) for isk = 0, isk >= r or a secret that is not the key's."""

    def __init__(self, verifier, isk):
        self.verifier = verifier
        self.curve = verifier.curve
        h = C.c_void_p()
        L.check("fts_idemix_issuer_create", L.lib.fts_idemix_issuer_create(verifier.h, _z32(isk), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            L.lib.fts_idemix_issuer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def issue(self, reqs, attrs, seed=None, stride=None):
        """reqs: n CredRequest protos (None: a NULL pointer); attrs: n lists of four ints or
        32-byte strings (None: a NULL pointer); seed None: the secure source, else test-only.
        -> (credentials: Credential protos, b"" for a rejected item; int32 status array:
        FTS_OK, FTS_E_SIGN_BADKEY or FTS_E_CREDREQ_*)"""
        n = len(reqs)
        if len(attrs) != n:
            raise ValueError("reqs and attrs must have the same length")
        ln = FTS_IDEMIX_CREDENTIAL_LEN
        stride = ln if stride is None else int(stride)
        st = np.zeros(n, dtype=np.int32)
        keep = []
        for r, a in zip(reqs, attrs):
            if a is not None and len(a) != 4:
                raise ValueError("four attributes per credential")
            keep.append((None if r is None else bytes(r), None if a is None else b"".join(_z32(v) for v in a)))
        items = (L.CredIssueItem * max(1, n))()
        for i, (r, a) in enumerate(keep):
            items[i].req = None if r is None else C.cast(C.c_char_p(r), C.c_void_p)
            items[i].req_len = len(r or b"")
            items[i].attrs4x32 = None if a is None else C.cast(C.c_char_p(a), C.c_void_p)
        out = np.zeros(max(1, n * stride), dtype=np.uint8)
        lens = np.zeros(max(1, n), dtype=np.uint32)
        sd = OS_RANDOM if seed is None else int(seed) & ((1 << 64) - 1)
        L.check("fts_idemix_cred_issue_batch",
                L.lib.fts_idemix_cred_issue_batch(self.h, n, items, sd, out.ctypes.data, stride, lens.ctypes.data,
                                                  st.ctypes.data_as(C.POINTER(C.c_int32))))
        raw = out.tobytes()
        self.last_buffer = raw[:n * stride]  # rejected items: zeros
        return [raw[i * stride:i * stride + int(lens[i])] for i in range(n)], st

    def last_timings(self):
        """(decode + products + check ms, A = inv B ms, host parse + draws + staging s, host
        serialisation s) of the last issue"""
        ms, hs = (C.c_float * 2)(), (C.c_double * 2)()
        L.check("fts_idemix_cred_issue_last_timings", L.lib.fts_idemix_cred_issue_last_timings(self.h, ms, hs))
        return float(ms[0]), float(ms[1]), float(hs[0]), float(hs[1])


def cred_issue_draws(curve, seed, i, avoid_e=None):
    """host-only: (E, S) of Issuer.issue's item i at `seed` and rSk of make_cred_requests' item i,
    as ints; avoid_e: the value r - isk that E is drawn again on"""
    out = (C.c_uint8 * 96)()
    L.check("fts_debug_idemix_cred_issue_draws",
            L.lib.fts_debug_idemix_cred_issue_draws(int(curve), int(seed), int(i),
                                                    None if avoid_e is None else _z32(avoid_e), out))
    b = bytes(out)
    return tuple(int.from_bytes(b[32 * k:32 * k + 32], "big") for k in range(3))


def parse_cred_request(curve, req):
    """host-only: the host's part of CredRequest.Check (fts_debug_idemix_credreq_parse) ->
    (status, Nym as X || Y, issuer_nonce, proof_c as sent, proof_s mod r)"""
    st, out = C.c_int32(), (C.c_uint8 * 160)()
    r = None if req is None else bytes(req)
    L.check("fts_debug_idemix_credreq_parse",
            L.lib.fts_debug_idemix_credreq_parse(int(curve), None if r is None else C.cast(C.c_char_p(r), C.c_void_p),
                                                 len(r or b""), C.byref(st), out))
    b = bytes(out)
    return st.value, b[:64], b[64:96], int.from_bytes(b[96:128], "big"), int.from_bytes(b[128:], "big")


def write_cred_request(nym_xy, nonce, c, s):
    """host-only: the CredRequest writer (nym_xy: (x, y) ints)"""
    out = (C.c_uint8 * FTS_IDEMIX_CRED_REQUEST_LEN)()
    L.check("fts_debug_idemix_credreq_write",
            L.lib.fts_debug_idemix_credreq_write(_z32(nym_xy[0]) + _z32(nym_xy[1]), _z32(nonce), _z32(c), _z32(s), out))
    return bytes(out)


def write_credential(a_xy, b_xy, e, s, attrs):
    """host-only: the Credential writer (a_xy, b_xy: (x, y) ints; four attributes)"""
    out = (C.c_uint8 * FTS_IDEMIX_CREDENTIAL_LEN)()
    L.check("fts_debug_idemix_credential_write",
            L.lib.fts_debug_idemix_credential_write(_z32(a_xy[0]) + _z32(a_xy[1]), _z32(b_xy[0]) + _z32(b_xy[1]),
                                                    _z32(e), _z32(s), b"".join(_z32(v) for v in attrs), out))
    return bytes(out)


class IssuerKeyError(Exception):
    def __init__(self, msg, status, index):
        super().__init__(msg)
        self.status = status
        self.index = index


def check_issuer_keys(ipks, curve, device=0, raise_on_error=False, return_hashes=False):
    """IssuerPublicKey.Check for a list of IssuerPublicKey protos (None: a NULL pointer) on the
    device (fts_idemix_ipk_check_batch; no handle).  -> int32 status array: FTS_OK or
    FTS_E_IPK_MALFORMED / _UNDEFINED / _PROOF; with return_hashes also the n hashes (HashToZr of
    each key without its hash field, 32 bytes).  raise_on_error: IssuerKeyError for the first
    bad key, carrying the reference's message.  The handles (IssuerKey, IdentityVerifier, Issuer)
    do not run this check: a caller that wants the reference's import semantics runs it first."""
    keep = [None if k is None else bytes(k) for k in ipks]
    n = len(keep)
    ptrs = (C.c_void_p * max(1, n))()
    lens = (C.c_size_t * max(1, n))()
    for i, k in enumerate(keep):
        ptrs[i] = None if k is None else C.cast(C.c_char_p(k), C.c_void_p)
        lens[i] = len(k or b"")
    st = np.zeros(n, dtype=np.int32)
    hs = np.zeros(max(1, n * 32), dtype=np.uint8)
    L.check("fts_idemix_ipk_check_batch",
            L.lib.fts_idemix_ipk_check_batch(int(device), int(curve), n, ptrs, lens,
                                             st.ctypes.data_as(C.POINTER(C.c_int32)), hs.ctypes.data))
    if raise_on_error:
        for i, s in enumerate(st):
            if s != FTS_OK:
                raise IssuerKeyError(L.status_str(s), int(s), i)
    if return_hashes:
        raw = hs.tobytes()
        return st, [raw[32 * i:32 * i + 32] for i in range(n)]
    return st


def generate_issuer_keys(n, curve, seed=None, device=0, stride=None):
    """NewIssuerKey n times on the device (fts_idemix_issuer_keygen_batch), attribute names OU,
    Role, EnrollmentID, RevocationHandle.  seed None: the secure source, else test-only (key i
    draws from seed + i).  -> [(isk as an int, IssuerPublicKey proto)]"""
    stride = FTS_IDEMIX_IPK_LEN if stride is None else int(stride)
    isk = np.zeros(max(1, n * 32), dtype=np.uint8)
    out = np.zeros(max(1, n * stride), dtype=np.uint8)
    lens = np.zeros(max(1, n), dtype=np.uint32)
    sd = OS_RANDOM if seed is None else int(seed) & ((1 << 64) - 1)
    L.check("fts_idemix_issuer_keygen_batch",
            L.lib.fts_idemix_issuer_keygen_batch(int(device), int(curve), n, sd, isk.ctypes.data, out.ctypes.data,
                                                 stride, lens.ctypes.data))
    ib, raw = isk.tobytes(), out.tobytes()
    return [(int.from_bytes(ib[32 * i:32 * i + 32], "big"), raw[i * stride:i * stride + int(lens[i])])
            for i in range(n)]


def issuer_key_last_kernel_ms():
    """(HIP-event ms of this process's last check_issuer_keys call, of its last generate_issuer_keys call)"""
    ms = (C.c_float * 2)()
    L.check("fts_idemix_issuer_key_last_timings", L.lib.fts_idemix_issuer_key_last_timings(ms))
    return float(ms[0]), float(ms[1])


def keygen_draws(curve, seed, i):
    """host-only: key i's draws at `seed` as ints, in the order isk, HSk, HRand, HAttrs[0..3],
    BarG1, r (the nine generate_issuer_keys consumes), then the stream's next value"""
    out = (C.c_uint8 * 320)()
    L.check("fts_debug_idemix_keygen_draws", L.lib.fts_debug_idemix_keygen_draws(int(curve), int(seed), int(i), out))
    b = bytes(out)
    return [int.from_bytes(b[32 * k:32 * k + 32], "big") for k in range(10)]


def parse_issuer_key(curve, ipk):
    """host-only: the host's part of the check (fts_debug_idemix_ipk_parse) -> (status, hash)"""
    st, out = C.c_int32(), (C.c_uint8 * 32)()
    k = None if ipk is None else bytes(ipk)
    L.check("fts_debug_idemix_ipk_parse",
            L.lib.fts_debug_idemix_ipk_parse(int(curve), None if k is None else C.cast(C.c_char_p(k), C.c_void_p),
                                             len(k or b""), C.byref(st), out))
    return st.value, bytes(out)


class IdentityError(Exception):
    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status


def _pb_top_fields(raw):
    """(field, wire type, value) of a proto's top level: varints and length-delimited
    fields only (what IdemixSignerConfig carries)"""
    out, i, n = [], 0, len(raw)

    def varint():
        nonlocal i
        v = sh = 0
        while True:
            if i >= n or sh > 63:
                raise ValueError("truncated proto")
            c = raw[i]
            i += 1
            v |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                return v
    while i < n:
        key = varint()
        f, wt = key >> 3, key & 7
        if wt == 0:
            out.append((f, wt, varint()))
        elif wt == 2:
            ln = varint()
            if ln > n - i:
                raise ValueError("truncated proto")
            out.append((f, wt, raw[i:i + ln]))
            i += ln
        else:
            raise ValueError("unsupported wire type %d" % wt)
    return out


def parse_signer_config(raw):
    """IdemixSignerConfig (the proto, or the JSON form idemixgen writes) ->
    (Credential proto, sk as 32 big-endian bytes, CredentialRevocationInformation or None)"""
    import base64
    import json
    raw = bytes(raw)
    try:
        j = json.loads(raw)
        cred, sk = base64.b64decode(j["Cred"]), base64.b64decode(j["Sk"])
        cri = base64.b64decode(j.get("credential_revocation_information", ""))
    except (ValueError, UnicodeDecodeError):
        f = {k: v for k, wt, v in _pb_top_fields(raw) if wt == 2}
        cred, sk, cri = f.get(1, b""), f.get(2, b""), f.get(6, b"")
    if len(sk) > 32:
        raise ValueError("user secret wider than 32 bytes")
    return cred, sk.rjust(32, b"\0"), (cri or None)


class GeneratedIdentities:
    """what Credential.generate returns: ids (serialized identities, b"" for a rejected item),
    rnym / r_eid / r_rh (32 big-endian bytes each) and the int32 status array"""

    def __init__(self, ids, rnym, r_eid, r_rh, status):
        self.ids, self.rnym, self.r_eid, self.r_rh, self.status = ids, rnym, r_eid, r_rh, status

    def __len__(self):
        return len(self.ids)


class Credential:
    """One wallet's idemix credential on the device (fts_idemix_cred): generate(n) yields what
    n calls of KeyManager.Identity do (services/identity/idemix/km.go:173-290) -- fresh owner
    identities with their association proof, the nym randomness for NymSigner and the audit
    randoms.  Borrows `verifier` (an IdentityVerifier under the credential's issuer key),
    which must stay open while this handle lives."""

    def __init__(self, verifier, cred, sk, cri=None):
        """cred: the Credential proto; sk: int or 32 big-endian bytes; cri: the
        CredentialRevocationInformation proto or None (epoch 0, the G2 generator)"""
        self.verifier = verifier
        self.curve = verifier.curve
        sk = sk.to_bytes(32, "big") if isinstance(sk, int) else bytes(sk)
        if len(sk) != 32:
            raise ValueError("the user secret is an int or 32 big-endian bytes")
        cred = bytes(cred)
        cri = None if cri is None else bytes(cri)
        h = C.c_void_p()
        L.check("fts_idemix_cred_create",
                L.lib.fts_idemix_cred_create(verifier.h, cred, len(cred), sk, cri, len(cri or b""), C.byref(h)))
        self.h = h

    @classmethod
    def from_signer_config(cls, verifier, raw, with_cri=True):
        cred, sk, cri = parse_signer_config(raw)
        return cls(verifier, cred, sk, cri if with_cri else None)

    def close(self):
        if getattr(self, "h", None):
            L.lib.fts_idemix_cred_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def identity_len(self):
        return int(L.lib.fts_idemix_identity_len(self.h))

    def generate(self, n, seed=None, r_eid=None, r_rh=None, id_stride=None):
        """n identities in one device pass -> GeneratedIdentities.  seed None: the secure
        source, else test-only (item i equals the one-item call at seed + i).  r_eid / r_rh:
        n ints or 32-byte strings (or one, repeated) that fix the audit randoms."""
        ln = self.identity_len
        stride = ln if id_stride is None else int(id_stride)
        st = np.zeros(n, dtype=np.int32)

        def fixed(v):
            if v is None:
                return None, None
            vs = list(v) if isinstance(v, (list, tuple)) else [v] * n
            if len(vs) != n:
                raise ValueError("a fixed audit random per identity")
            b = b"".join((x.to_bytes(32, "big") if 0 <= x < (1 << 256) else b"\xff" * 32) if isinstance(x, int)
                         else bytes(x) for x in vs)
            if len(b) != 32 * n:
                raise ValueError("an audit random is an int or 32 big-endian bytes")
            a = np.frombuffer(b, dtype=np.uint8)
            return a, a.ctypes.data
        keep_e, p_e = fixed(r_eid)
        keep_r, p_r = fixed(r_rh)
        ids = np.zeros(max(1, n * stride), dtype=np.uint8)
        lens = np.zeros(max(1, n), dtype=np.uint32)
        rn, re_, rr = (np.zeros(max(1, 32 * n), dtype=np.uint8) for _ in range(3))
        sd = OS_RANDOM if seed is None else int(seed) & ((1 << 64) - 1)
        L.check("fts_idemix_identity_generate_batch",
                L.lib.fts_idemix_identity_generate_batch(self.h, n, sd, p_e, p_r, ids.ctypes.data, stride,
                                                         lens.ctypes.data, rn.ctypes.data, re_.ctypes.data,
                                                         rr.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_int32))))
        raw = ids.tobytes()
        cut = lambda a: [a[32 * i:32 * i + 32].tobytes() for i in range(n)]  # noqa: E731
        return GeneratedIdentities([raw[i * stride:i * stride + int(lens[i])] for i in range(n)],
                                   cut(rn), cut(re_), cut(rr), st)

    def draws(self, seed, i):
        """the 18 scalars of item i at `seed` (fts_debug_idemix_identity_draws), as ints:
        rnym, r1, r2, nonce, rSk, rE, rR2, rR3, rS', rRNym, rAttrs[0..3], r_eid, r_rh, rr_eid, rr_rh"""
        return identity_draws(self.curve, seed, i)

    def last_timings(self):
        """(k_idg_prep + k_idg_points ms, k_idg_finish ms, host draw + staging s, host serialisation s)"""
        ms, hs = (C.c_float * 2)(), (C.c_double * 2)()
        L.check("fts_idemix_identity_generate_last_timings",
                L.lib.fts_idemix_identity_generate_last_timings(self.h, ms, hs))
        return float(ms[0]), float(ms[1]), float(hs[0]), float(hs[1])


def identity_draws(curve, seed, i):
    """host-only: the draws of Credential.generate's item i at `seed` on `curve`"""
    out = (C.c_uint8 * (18 * 32))()
    L.check("fts_debug_idemix_identity_draws",
            L.lib.fts_debug_idemix_identity_draws(int(curve), int(seed), int(i), out))
    b = bytes(out)
    return [int.from_bytes(b[32 * k:32 * k + 32], "big") for k in range(18)]


def write_identity(curve, points, scalars, nonce, epoch_pk=None, epoch=0):
    """host-only: the identity writer on given values (fts_debug_idemix_identity_write).
    points: A' ABar B' Nym EidNym RhNym as (x, y); scalars: c sSk sE sR2 sR3 sS' sAttrs[0..3]
    sRNym sEid sRh; epoch_pk: 128 raw bytes in the curve's ECP2 order, None: the generator"""
    pts = b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in points)
    sc = b"".join(s.to_bytes(32, "big") for s in scalars)
    if len(pts) != 384 or len(sc) != 416:
        raise ValueError("six points and thirteen scalars")
    n = C.c_size_t()
    buf = (C.c_uint8 * 2048)()
    L.check("fts_debug_idemix_identity_write",
            L.lib.fts_debug_idemix_identity_write(int(curve), pts, sc, nonce.to_bytes(32, "big"), epoch_pk, int(epoch),
                                                  buf, 2048, C.byref(n)))
    return bytes(buf[:n.value])


class AuditMatchError(Exception):
    def __init__(self, msg, status):
        super().__init__(msg)
        self.status = status
