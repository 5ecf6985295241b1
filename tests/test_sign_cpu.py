"""CPU: the parts of signing that run on the host -- the RFC 6979 HMAC-DRBG that
k_ecdsa_sign runs per lane (csrc/common/hmac_drbg.hpp) and the two encoders
(csrc/host/sign_encode.hpp), through lib/sign_check (a stand-alone program built
with the host address and undefined-behaviour sanitizers), and the host-only entry
points through ctypes."""
import ctypes as C
import os
import random
import subprocess

import pytest

from conftest import PKG

import sign_ref as R
from oracle import ecdsa_p256 as E
from oracle import idemix as O

CHECK = os.path.join(PKG, "lib", "sign_check")
HALF = E.N >> 1
EDGES = [1, 0x7F, 0x80, 1 << 247, (1 << 248) - 1, 1 << 255]
R_EDGES, S_EDGES = EDGES + [E.N - 1], EDGES + [HALF]


def run(lines):
    p = subprocess.run([CHECK], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def h32(v):
    return "%064x" % v


def test_rfc6979_a25_nonces():
    out = run(["km %s %s" % (h32(R.RFC_KEY), m.hex()) for m in (b"sample", b"test")])
    assert out == ["a6e3c57dd01abe90086538398355dd4c3b17aa873382b0f24d6129493d8aad60",
                   "d16b6ae827f17175e040871a1c7ec3500192c4c92677336ec2537acaee0008e0"]
    # the test's own RFC 6979 against the same vectors
    assert [h32(R.nonce(R.RFC_KEY, m)) for m in (b"sample", b"test")] == out


def _triples():
    rng = random.Random(6979)
    t = []
    for i in range(200):
        d = rng.choice([1, E.N - 1, rng.randrange(1, 1 << 128), rng.randrange(1, E.N), rng.randrange(1, E.N)])
        # digests >= n (bits2octets reduces them): every fifth one, and the ends of that range
        h = rng.randrange(E.N, 1 << 256) if i % 5 == 0 else rng.randrange(1 << 256)
        h = {11: E.N, 21: (1 << 256) - 1, 31: E.N - 1, 41: 0}.get(i, h)
        extra = rng.randbytes(32) if i % 2 else b""
        t.append((d, h.to_bytes(32, "big"), extra))
    return t


def test_nonce_against_hmac_reference():
    t = _triples()
    assert sum(int.from_bytes(h, "big") >= E.N for _, h, _ in t) >= 40
    out = run(["k %s %s %s" % (h32(d), h.hex(), x.hex()) for d, h, x in t])
    for (d, h, x), got in zip(t, out):
        assert got == h32(next(R.candidates(d, h, x))), (d, h.hex(), x.hex())


def test_retry_step_against_hmac_reference():
    # the candidates that follow a rejected one (r = 0 or s = 0): K = HMAC_K(V || 0x00), V = HMAC_K(V)
    t = _triples()[:20]
    out = run(["k3 %s %s %s" % (h32(d), h.hex(), x.hex()) for d, h, x in t])
    for (d, h, x), got in zip(t, out):
        g = R.candidates(d, h, x)
        assert got.split() == [h32(next(g)) for _ in range(3)]


def test_der_encoding_and_back():
    from fts_gpu import ecdsa as G
    pairs = [(r, s) for r in R_EDGES for s in S_EDGES]
    out = run(["der %s %s" % (h32(r), h32(s)) for r, s in pairs])
    for (r, s), got in zip(pairs, out):
        der = bytes.fromhex(got)
        assert der == E.der_sig(r, s), (r, s)
        assert len(der) <= 72
        assert G.parse_sig(der) == (G.FTS_OK if s <= HALF else G.FTS_E_SIG_NOT_LOW_S, r, s)
        assert G.sig_encode(r, s) == der  # fts_ecdsa_sig_encode through ctypes
    assert max(len(bytes.fromhex(o)) for o in out) == 72


def test_nym_proto_writer():
    rng = random.Random(136)
    for C_ in (O.BN254C, O.FP256BNC):
        vals = [0, 1, C_.r - 1] + [rng.randrange(C_.r) for _ in range(5)]
        quads = [(vals[i % 8], vals[(i + 1) % 8], vals[(i + 3) % 8], vals[(i + 5) % 8]) for i in range(8)]
        out = run(["nym " + " ".join(h32(v) for v in q) for q in quads])
        for q, got in zip(quads, out):
            raw = bytes.fromhex(got)
            assert len(raw) == 136 and raw == O.encode_nym_sig(*q)
            assert O.decode_nym_sig(raw, C_) == q


def test_padded_stream_words_against_sha256():
    # the nym and audit kernels' padded_word / padded_blocks on the host: every tail length
    # 0..200 behind no prefix (FP256BN, audit) and behind the 164-byte BN254 prefix, so every
    # residue mod 64 of the total, the 55/56 and 63/0 edges among them, several times over
    import hashlib
    rng = random.Random(164)
    cases = [(rng.randbytes(pre), rng.randbytes(ln)) for pre in (0, 164) for ln in range(201)]
    out = run(["pad %s %s" % (p.hex() or "-", t.hex() or "-") for p, t in cases])
    for (p, t), got in zip(cases, out):
        assert got == hashlib.sha256(p + t).hexdigest(), (len(p), len(t))


def test_padded_block_count_does_not_wrap():
    # the longest stream the API takes: (len + 72) / 64 wraps in 32 bits there
    lens = [0, 55, 56, 63, 64, 119, 120, 0xFFFFFF00 + 166, 0xFFFFFFFF]
    out = run(["blocks %08x" % n for n in lens])
    assert [int(o, 16) for o in out] == [(n + 9 + 63) // 64 for n in lens]


def test_sign_entry_points_argument_errors():
    from fts_gpu import _lib as L
    lib = L.lib
    EINVAL = lib.fts_ecdsa_sig_encode(None, None, None, None)
    assert EINVAL != L.FTS_API_OK
    # n = 0 is a no-op, whatever the pointers (and needs no device)
    for mode in (L.FTS_NONCE_RFC6979, L.FTS_NONCE_HEDGED):
        assert lib.fts_ecdsa_sign_batch(0, 0, None, mode, 0, None, None, None) == L.FTS_API_OK
    assert lib.fts_ecdsa_sign_batch(0, 0, None, 2, 0, None, None, None) == EINVAL  # unknown nonce mode
    item = (L.EcdsaSignItem * 1)()
    sig, ln, st = (C.c_uint8 * 72)(), (C.c_uint32 * 1)(), (C.c_int32 * 1)()
    I32 = C.POINTER(C.c_int32)
    assert lib.fts_ecdsa_sign_batch(0, 1, None, 0, 0, sig, ln, C.cast(st, I32)) == EINVAL
    assert lib.fts_ecdsa_sign_batch(0, 1, item, 0, 0, None, ln, C.cast(st, I32)) == EINVAL
    assert lib.fts_ecdsa_sign_batch(0, 1, item, 0, 0, sig, None, C.cast(st, I32)) == EINVAL
    assert lib.fts_ecdsa_sign_batch(0, 1, item, 0, 0, sig, ln, None) == EINVAL
    assert lib.fts_ecdsa_sign_batch(-1, 1, item, 0, 0, sig, ln, C.cast(st, I32)) == EINVAL
    assert lib.fts_ecdsa_sign_batch(0, (1 << 24) + 1, item, 0, 0, sig, ln, C.cast(st, I32)) == EINVAL
    assert lib.fts_ecdsa_sign_last_timings(0, None) == EINVAL
    r32 = (1).to_bytes(32, "big")
    n = C.c_uint32()
    assert lib.fts_ecdsa_sig_encode(r32, r32, sig, None) == EINVAL
    assert lib.fts_ecdsa_sig_encode(None, r32, sig, C.byref(n)) == EINVAL
    assert lib.fts_ecdsa_sig_encode(r32, r32, sig, C.byref(n)) == L.FTS_API_OK and n.value == 8
    # a nym signature needs an issuer-key handle
    nsig = (C.c_uint8 * 136)()
    assert lib.fts_nym_sign_batch(None, 0, None, 0, None, None) == EINVAL
    assert lib.fts_nym_sign_batch(None, 1, (L.NymSignItem * 1)(), 0, nsig, C.cast(st, I32)) == EINVAL
    assert lib.fts_nym_sign_last_timings(None, None) == EINVAL


def test_status_string():
    from fts_gpu import _lib as L
    assert L.FTS_E_SIGN_BADKEY == 34
    assert L.status_str(L.FTS_E_SIGN_BADKEY) == "signing key out of range"
    assert L.status_str(35) == "unknown status"


def test_python_mirror_rejects_bad_arguments():
    from fts_gpu import ecdsa as G
    assert G.sign_batch([], []) == []
    with pytest.raises(ValueError):
        G.sign_batch([b"m"], [])
    with pytest.raises(ValueError):
        G.sign_batch([b"m"], [1], mode="random")
    with pytest.raises(ValueError):
        G.sign_batch([b"m"], [b"short"])
