"""GPU: signing on the device -- fts_ecdsa_sign_batch (ecdsa.Signer.Sign,
validator/ecdsa/ecdsa.go:49-63, with RFC 6979 nonces) and fts_nym_sign_batch (the idemix
nym signer, IBM/idemix NewNymSignature) on both curves.

ECDSA signatures are compared byte for byte with oracle.ecdsa_p256.sign at the nonce
of the test's own RFC 6979 (sign_ref.py); nym signatures are accepted by
oracle.idemix.nym_verify and reproduced by oracle.idemix.nym_sign from the nonces
recovered out of them.  Every signature is also fed back to the library's verifiers.

Every case takes a few seconds but the FP256BN oracle comparison: oracle/idemix.py inverts
by Fermat in every point addition (tens of ms per scalar product, 8 of them per item in
nym_verify twice and nym_sign once), so its 300 items take about a minute of host time
(62 s measured); the device's share of that case is milliseconds."""
import json
import os
import random
import threading

import pytest

from conftest import GOLDEN

import sign_ref as R
from oracle import ecdsa_p256 as E
from oracle import idemix as O

pytestmark = pytest.mark.gpu

N = E.N
HALF = N >> 1
ECDSA_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 300, 2000]
NYM_LENS = [0, 1, 17, 18, 19, 20, 25, 26, 27, 28, 29, 300, 1024]

with open(os.path.join(GOLDEN, "idemix_golden.json")) as f:
    GOLD = json.load(f)


def pub(d):
    return E.mul(d, E.G)


# --------------------------------------------------------------------- ECDSA
def test_ecdsa_known_answers():
    from fts_gpu import ecdsa as G
    sigs = G.sign_batch([b"sample", b"test"], [R.RFC_KEY] * 2, mode="rfc6979")
    want = [(0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
             0x0834E36AD29A83BF2BC9385E491D6099C8FDF9D1ED67AA7EA5F51F93782857A9),
            (0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
             0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083)]
    assert [E.parse_sig(s) for s in sigs] == want
    assert sigs == [E.der_sig(*w) for w in want]
    # the RFC's s for "sample" is the high one
    assert N - want[0][1] == 0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8


def _ecdsa_batch():
    """300 (key, message) pairs whose raw s falls on both sides of n/2 often enough,
    their RFC 6979 nonces, and the first "zero-window-%d" message whose nonce has a zero
    16-bit window"""
    for seed in range(1000, 1010):
        rng = random.Random(seed)
        keys = [rng.randrange(1, N) for _ in range(8)] + [1, N - 1, rng.randrange(1, 1 << 128)]
        ds = [keys[rng.randrange(len(keys))] for _ in range(300)]
        ds[:len(keys)] = keys  # every key at least once
        msgs = [rng.randbytes(ECDSA_LENS[i % len(ECDSA_LENS)]) for i in range(300)]
        ks = [R.nonce(d, m) for d, m in zip(ds, msgs)]
        high = sum(R.raw_s(d, m, k) > HALF for d, m, k in zip(ds, msgs, ks))
        if 50 <= high <= 250:
            break
    else:
        raise AssertionError("no seed gives both low-S branches")
    zd = keys[0]
    for j in range(200000):
        zm = b"zero-window-%d" % j
        zk = R.nonce(zd, zm)
        if any((zk >> (16 * w)) & 0xFFFF == 0 for w in range(16)):
            break
    else:
        raise AssertionError("no nonce with a zero window in 200,000 tries")
    return ds + [zd], msgs + [zm], ks + [zk], high


@pytest.fixture(scope="module")
def ecdsa_batch():
    return _ecdsa_batch()


@pytest.fixture(scope="module")
def pubs(ecdsa_batch):
    cache = {}
    return [cache.setdefault(d, pub(d)) for d in ecdsa_batch[0]]


def test_ecdsa_batch_matches_oracle(ecdsa_batch, pubs):
    from fts_gpu import ecdsa as G
    ds, msgs, ks, high = ecdsa_batch
    assert len(ds) == 301 and 50 <= high <= 250
    sigs, st = G.sign_batch(msgs, ds, mode="rfc6979", return_status=True)
    assert not st.any()
    for i, (d, m, k, s) in enumerate(zip(ds, msgs, ks, sigs)):
        assert s == E.sign(d, m, k), i
    assert all(E.verify(m, s, p) == E.OK for m, s, p in zip(msgs, sigs, pubs))
    assert not G.verify_batch(msgs, sigs, pubs).any()
    # the seed is ignored in this mode
    assert G.sign_batch(msgs[:20], ds[:20], mode="rfc6979", seed=99) == sigs[:20]


def test_ecdsa_bad_keys_between_valid_ones(ecdsa_batch):
    from fts_gpu import ecdsa as G
    ds, msgs, ks, _ = ecdsa_batch
    ds, msgs, ks = list(ds[:7]), list(msgs[:7]), list(ks[:7])
    bad = {1: 0, 3: N, 5: (1 << 256) - 1}
    for i, d in bad.items():
        ds[i] = d
    sigs, st = G.sign_batch(msgs, ds, mode="rfc6979", return_status=True)
    for i in range(7):
        if i in bad:
            assert st[i] == G.FTS_E_SIGN_BADKEY and sigs[i] == b""
        else:
            assert st[i] == G.FTS_OK and sigs[i] == E.sign(ds[i], msgs[i], ks[i])
    sigs, st = G.sign_batch(msgs, ds, mode="hedged", seed=3, return_status=True)
    assert [int(s) for s in st] == [G.FTS_E_SIGN_BADKEY if i in bad else 0 for i in range(7)]
    assert all((s == b"") == (i in bad) for i, s in enumerate(sigs))
    with pytest.raises(G.SignatureError):
        G.Signer(0).Sign(b"m")


def test_ecdsa_hedged_mode(ecdsa_batch, pubs):
    from fts_gpu import ecdsa as G
    ds, msgs = ecdsa_batch[0][:300], ecdsa_batch[1][:300]
    pk = pubs[:300]

    def rs(sigs):
        return [E.parse_sig(s)[0] for s in sigs]
    det = G.sign_batch(msgs, ds, mode="rfc6979")
    a = G.sign_batch(msgs, ds, mode="hedged", seed=7)
    assert not G.verify_batch(msgs, a, pk).any()
    assert all(x != y for x, y in zip(rs(a), rs(det)))
    assert G.sign_batch(msgs, ds, mode="hedged", seed=7) == a
    for i in range(300):
        assert G.sign_batch([msgs[i]], [ds[i]], mode="hedged", seed=7 + i) == [a[i]], i
    b = G.sign_batch(msgs, ds, mode="hedged", seed=8)
    assert all(x != y for x, y in zip(rs(a), rs(b)))
    # the same seed and another message: another nonce
    c = G.sign_batch([m + b"!" for m in msgs], ds, mode="hedged", seed=7)
    assert all(x != y for x, y in zip(rs(a), rs(c)))
    # the default: hedged under the OS source
    o1, o2 = G.sign_batch(msgs, ds), G.sign_batch(msgs, ds)
    assert not G.verify_batch(msgs, o1, pk).any() and not G.verify_batch(msgs, o2, pk).any()
    assert not set(rs(o1)) & set(rs(o2))
    t = G.sign_last_timings()
    assert t["k_ecdsa_sign"] > 0 and t["k_ecdsa_digest"] > 0


# ----------------------------------------------------------------------- nym
CURVES = {"bn254": 1, "fp256bn": 0}


@pytest.fixture(scope="module", params=["bn254", "fp256bn"])
def nym_case(request):
    """the device handle, the oracle's key, and 300 seeded (sk, rnym, Nym, message) items"""
    from fts_gpu import idemix as I
    name = request.param
    C = O.CURVES[CURVES[name]]
    raw = bytes.fromhex(GOLD[name]["ipk"])
    ipk = O.parse_ipk(raw, C)
    dev = I.IssuerKey(raw, device=0, curve=CURVES[name])
    rng = random.Random(254 + CURVES[name])
    sks = [rng.randrange(C.r) for _ in range(300)]
    rns = [rng.randrange(C.r) for _ in range(300)]
    sks[0], rns[1], sks[2], rns[2] = 0, 0, C.r - 1, C.r - 1
    nyms = [O.nym_bytes(ipk, O.make_nym(ipk, a, b)) for a, b in zip(sks, rns)]
    msgs = [rng.randbytes(NYM_LENS[i % len(NYM_LENS)]) for i in range(300)]
    yield {"C": C, "ipk": ipk, "dev": dev, "sks": sks, "rns": rns, "nyms": nyms, "msgs": msgs}
    dev.close()


class _Stub:
    def __init__(self, vals):
        self.vals = list(vals)

    def randrange(self, _):
        return self.vals.pop(0)


def test_nym_batch_matches_oracle(nym_case):
    c = nym_case
    C, ipk, dev = c["C"], c["ipk"], c["dev"]
    sigs, st = dev.sign_batch(c["sks"], c["rns"], c["nyms"], c["msgs"], seed=11, return_status=True)
    assert not st.any() and all(len(s) == 136 for s in sigs)
    for i, (sk, rn, nym, m, sig) in enumerate(zip(c["sks"], c["rns"], c["nyms"], c["msgs"], sigs)):
        O.nym_verify(ipk, nym, sig, m)
        with pytest.raises(O.NymError):
            O.nym_verify(ipk, nym, sig, m + b"!")
        ch, s_sk, s_r, nonce = O.decode_nym_sig(sig, C)
        assert max(ch, s_sk, s_r, nonce) < C.r
        stub = _Stub([nonce, (s_sk - ch * sk) % C.r, (s_r - ch * rn) % C.r])
        assert O.nym_sign(ipk, sk, C.g1_from_bytes(nym), rn, m, stub) == sig, i
    assert not dev.verify_batch(c["nyms"], sigs, c["msgs"]).any()
    assert dev.last_sign_kernel_ms() > 0


def test_nym_determinism(nym_case):
    c = nym_case
    C, dev = c["C"], c["dev"]
    args = (c["sks"], c["rns"], c["nyms"], c["msgs"])

    def nonces(sigs):
        return [O.decode_nym_sig(s, C)[3] for s in sigs]
    a = dev.sign_batch(*args, seed=11)
    assert dev.sign_batch(*args, seed=11) == a
    for i in range(300):
        assert dev.sign_batch(*[x[i:i + 1] for x in args], seed=11 + i) == [a[i]], i
    b = dev.sign_batch(*args, seed=12)
    assert all(x != y for x, y in zip(nonces(a), nonces(b)))
    o1, o2 = dev.sign_batch(*args), dev.sign_batch(*args)  # the OS source
    assert not dev.verify_batch(c["nyms"], o1, c["msgs"]).any()
    assert not dev.verify_batch(c["nyms"], o2, c["msgs"]).any()
    assert not set(nonces(o1)) & set(nonces(o2))


def test_nym_bad_items_between_valid_ones(nym_case):
    from fts_gpu import idemix as I
    c = nym_case
    C, dev = c["C"], c["dev"]
    sks, rns, nyms, msgs = (list(c[k][:9]) for k in ("sks", "rns", "nyms", "msgs"))
    good = dev.sign_batch(sks, rns, nyms, msgs, seed=21)
    sks[1] = C.r                      # sk = r
    rns[3] = (1 << 256) - 1           # rnym = 2^256 - 1
    off = bytearray(nyms[5])          # Nym off the curve
    off[-1] ^= 1
    nyms[5] = bytes(off)
    nyms[7] = nyms[7][:-1]            # one byte short
    sigs, st = dev.sign_batch(sks, rns, nyms, msgs, seed=21, return_status=True)
    want = {1: I.FTS_E_SIGN_BADKEY, 3: I.FTS_E_SIGN_BADKEY, 5: I.FTS_E_NYM_BADKEY, 7: I.FTS_E_NYM_BADKEY}
    assert [int(s) for s in st] == [want.get(i, 0) for i in range(9)]
    for i in range(9):
        assert sigs[i] == (b"" if i in want else good[i])


# ------------------------------------------------------------- shared slots
def test_six_threads_sign_and_verify(ecdsa_batch, pubs, nym_case):
    from fts_gpu import ecdsa as G
    ds, msgs, pk = ecdsa_batch[0][:300], ecdsa_batch[1][:300], pubs[:300]
    c = nym_case
    res = [None] * 6

    def work(t):
        try:
            s = G.sign_batch(msgs, ds, mode="hedged", seed=100 + t)
            ok = not G.verify_batch(msgs, s, pk).any()
            ns = c["dev"].sign_batch(c["sks"], c["rns"], c["nyms"], c["msgs"], seed=200 + t)
            res[t] = ok and not c["dev"].verify_batch(c["nyms"], ns, c["msgs"]).any()
        except Exception as e:  # reported by the assertion below
            res[t] = e
    th = [threading.Thread(target=work, args=(t,)) for t in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert res == [True] * 6


# --------------------------------------------------------------- end to end
def test_signed_request_end_to_end(nym_case):
    from fts_gpu import ecdsa as G, idemix as I, request as Q
    c = nym_case
    body = Q.token_request([(Q.TRANSFER, Q.transfer_action([(b"tx", 0, b"owner", bytes(64))], [(b"o", bytes(64))], b"p"))])
    d = 0x1234567890ABCDEF << 64 | 5
    s1 = G.Signer(d).Sign(body)
    sk, rn, nym = c["sks"][7], c["rns"][7], c["nyms"][7]
    s2 = I.NymSigner(c["dev"], sk, rn, nym).Sign(body)
    full = Q.token_request([(Q.TRANSFER, Q.transfer_action([(b"tx", 0, b"owner", bytes(64))], [(b"o", bytes(64))], b"p"))],
                           signatures=[s1, s2])
    assert full.startswith(body)
    got = [dict((f, v) for f, _, v in O.pb_fields(v))[1] for f, _, v in O.pb_fields(full) if f == 3]
    assert got == [s1, s2]
    G.Verifier(pub(d)).Verify(body, got[0])
    I.NymSignatureVerifier(c["dev"], nym).Verify(body, got[1])
    with pytest.raises(G.SignatureError):
        G.Verifier(pub(d)).Verify(body + b"!", got[0])
    with pytest.raises(I.SignatureError):
        I.NymSignatureVerifier(c["dev"], nym).Verify(body + b"!", got[1])
