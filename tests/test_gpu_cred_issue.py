"""GPU: idemix enrolment on the device, on both curves -- credential requests made
(fts_idemix_cred_request_batch) and checked (fts_idemix_cred_request_verify_batch), credentials
issued (fts_idemix_issuer, fts_idemix_cred_issue_batch): byte-exact against the restatement of
tests/cred_issue_ref.py at the library's draws; the whole loop request -> credential ->
identities -> verified identities under the reference's own BN254 issuer secret and under a
made FP256BN key; wrong secrets; the redraw of an E with E + isk = 0; the verdicts over every
tampering; the API edges, two threads on one handle and the edge of a tile of 16,384.

One restated batch of 257 items per curve is computed once and shared: item i of a call
depends on (seed + i, its own inputs) alone, so every shorter batch is a prefix of it."""
import ctypes as C
import functools
import random
import threading

import numpy as np
import pytest

import cred_issue_ref as R
from oracle import idemix as OI

pytestmark = pytest.mark.gpu

TAGS = ["bn254", "fp256bn"]
API_EPP, API_ESIZE = -2, -5
PAIRING = 38
SEED_REQ, SEED_ISS, NREF = 9100, 9200, 257
OTHER = {"bn254": "bn254_charlie", "fp256bn": "fp256bn_validator"}  # another issuer key of the curve


@functools.lru_cache(maxsize=None)
def key(tag):
    """-> (isk, IssuerPublicKey proto, parsed key): the reference's own on BN254, a made one on FP256BN"""
    isk, raw = R.tokengen() if tag == "bn254" else R.make_issuer_key(tag, random.Random(4100))
    return isk, raw, OI.parse_ipk(raw, R.CURVES[tag][1])


@pytest.fixture(scope="module")
def handles():
    from fts_gpu import idemix as I
    hs = {}
    for tag in TAGS:
        isk, raw, _ = key(tag)
        V = I.IdentityVerifier(raw, device=0, curve=R.CURVES[tag][0])
        hs[tag] = (V, I.Issuer(V, isk))
    yield hs
    for V, S in hs.values():
        S.close()
        V.close()


@functools.lru_cache(maxsize=None)
def ref(tag):
    """NREF restated items at the library's draws: sks (1 and r - 1 among them), nonces,
    attributes (0, 1 and r - 1 among them), requests, credential parts and protos"""
    from fts_gpu import idemix as I
    cid, Cv, _ = R.CURVES[tag]
    isk, _, ipk = key(tag)
    rng = random.Random(31 + cid)
    sks = [1, Cv.r - 1] + [rng.randrange(Cv.r) for _ in range(NREF - 2)]
    nonces = [rng.randbytes(32) for _ in range(NREF)]
    attrs = [[0, 1, Cv.r - 1, rng.randrange(Cv.r)]] + [[rng.randrange(Cv.r) for _ in range(4)] for _ in range(NREF - 1)]
    reqs, parts = [], []
    for i in range(NREF):
        reqs.append(R.new_cred_request(ipk, sks[i], nonces[i], I.cred_issue_draws(cid, SEED_REQ, i)[2]))
        E, S, _ = I.cred_issue_draws(cid, SEED_ISS, i)
        parts.append(R.new_credential(ipk, isk, reqs[i], attrs[i], E, S))
    return {"sks": sks, "nonces": nonces, "attrs": attrs, "reqs": reqs, "parts": parts,
            "creds": [R.cred_proto(k) for k in parts]}


def _ok(st):
    return [int(s) for s in st] == [0] * len(st)


# ------------------------------------------------- 1. byte-exact against the restatement
# lanes of the product kernel are laid out as product * n + item: an n that is no multiple of
# 64 makes a wave straddle two product kinds, and 255 / 256 / 257 are the block edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("tag", TAGS)
def test_byte_exact(handles, tag, n):
    V, S = handles[tag]
    r = ref(tag)
    reqs, st = V.make_cred_requests(r["sks"][:n], r["nonces"][:n], seed=SEED_REQ)
    assert _ok(st) and reqs == r["reqs"][:n]
    assert _ok(V.verify_cred_requests(reqs))
    creds, st = S.issue(reqs, r["attrs"][:n], seed=SEED_ISS)
    assert _ok(st) and creds == r["creds"][:n]
    assert all(len(c) == 344 for c in creds) and all(len(q) == 172 for q in reqs)


# ------------------------------------------------- 2. the enrolment loop
@pytest.mark.parametrize("tag", TAGS)
def test_issued_credentials_verify_and_yield_identities(handles, tag):
    """under the reference's own key (BN254) and a made key (FP256BN): Credential.Ver accepts
    what the device issued, fts_idemix_cred_create accepts it, its identities verify"""
    from fts_gpu import idemix as I
    V, S = handles[tag]
    r = ref(tag)
    n = 6
    reqs, st = V.make_cred_requests(r["sks"][:n], r["nonces"][:n])  # the secure source
    assert _ok(st)
    creds, st = S.issue(reqs, r["attrs"][:n])
    assert _ok(st)
    assert _ok(V.verify_credentials(creds, r["sks"][:n]))
    # another user's secret: the b-value does not match
    assert int(V.verify_credentials(creds[:1], [r["sks"][2]])[0]) == I.FTS_E_CRED_B
    for j in (0, 1, 5):
        cred = I.Credential(V, creds[j], r["sks"][j])
        try:
            g = cred.generate(3, seed=77 + j)
            assert _ok(g.status) and _ok(V.verify_batch(g.ids))
        finally:
            cred.close()


# ------------------------------------------------- 3. wrong secrets
@pytest.mark.parametrize("tag", TAGS)
def test_wrong_secret(handles, tag):
    from fts_gpu import idemix as I, _lib as L
    V, _ = handles[tag]
    Cv = R.CURVES[tag][1]
    isk, _, ipk = key(tag)
    for bad in (isk + 1, 0, Cv.r, (1 << 256) - 1):
        with pytest.raises(L.FtsError) as e:
            I.Issuer(V, bad)
        assert e.value.code == API_EPP
    # directly: a credential restated with isk + 1 fails the pairing equation, and only that
    r = ref(tag)
    k = R.new_credential(ipk, isk + 1, r["reqs"][3], r["attrs"][3], r["parts"][3]["E"], r["parts"][3]["S"])
    st = V.verify_credentials([R.cred_proto(k), r["creds"][3]], [r["sks"][3]] * 2)
    assert [int(s) for s in st] == [PAIRING, 0]


def test_key_without_bar_points_has_no_issuer(handles):
    """an IssuerPublicKey without BarG1 / BarG2 still makes a verifier, but no issuer"""
    from fts_gpu import idemix as I, _lib as L
    isk, raw, _ = key("bn254")
    cut = b"".join(OI.pb_bytes_field(f, v) for f, _, v in OI.pb_fields(raw) if f not in (6, 7))
    V = I.IdentityVerifier(cut, device=0, curve=1)
    try:
        with pytest.raises(L.FtsError) as e:
            I.Issuer(V, isk)
        assert e.value.code == API_EPP
    finally:
        V.close()


# ------------------------------------------------- 4. the redraw of E
def test_redraw_of_e_with_no_inverse():
    """a BN254 key with isk = r - E0, E0 the first draw of (seed, i): item i's credential is made
    at the item's second draw, still verifies, and its neighbours are where they were"""
    from fts_gpu import idemix as I
    cid, Cv, _ = R.CURVES["bn254"]
    seed, i, n = 5150, 2, 5
    E0 = I.cred_issue_draws(cid, seed, i)[0]
    isk, raw = R.make_issuer_key("bn254", random.Random(12), isk=Cv.r - E0)
    ipk = OI.parse_ipk(raw, Cv)
    rng = random.Random(13)
    sks = [rng.randrange(Cv.r) for _ in range(n)]
    attrs = [[rng.randrange(Cv.r) for _ in range(4)] for _ in range(n)]
    reqs = [R.new_cred_request(ipk, sk, rng.randbytes(32), rng.randrange(Cv.r)) for sk in sks]
    V = I.IdentityVerifier(raw, device=0, curve=cid)
    S = I.Issuer(V, isk)
    try:
        creds, st = S.issue(reqs, attrs, seed=seed)
        assert _ok(st) and _ok(V.verify_credentials(creds, sks))
        for j in range(n):
            E, Sd, _ = I.cred_issue_draws(cid, seed, j, avoid_e=E0 if j == i else None)
            assert E != E0
            if j == i:
                assert E == I.cred_issue_draws(cid, seed, j)[1]  # the second value of the stream
            assert creds[j] == R.cred_proto(R.new_credential(ipk, isk, reqs[j], attrs[j], E, Sd)), j
    finally:
        S.close()
        V.close()


# ------------------------------------------------- 5. verdicts
@functools.lru_cache(maxsize=None)
def verdict_batch(tag):
    """[(name, request or None, attributes or None, the request's verdict, the issue's verdict)]"""
    cid, Cv, _ = R.CURVES[tag]
    _, _, ipk = key(tag)
    r = ref(tag)
    req, at = r["reqs"][7], r["attrs"][7]
    nym, nonce, c, s = R._parse_request(ipk, req)
    other = OI.parse_ipk(R.raw(OTHER[tag], "IssuerPublicKey"), Cv)
    enc = R.encode_request
    f = OI.pb_fields(req)
    flip = bytes([nonce[0] ^ 1]) + nonce[1:]
    out = [("honest 0", r["reqs"][0], r["attrs"][0]), ("honest 7", req, at),
           ("tampered proof_c", enc(nym, nonce, (c + 1) % Cv.r, s), at),
           ("tampered proof_s", enc(nym, nonce, c, (s + 1) % Cv.r), at),
           ("tampered nonce", enc(nym, flip, c, s), at),
           ("tampered Nym", enc(Cv.add(nym, R.G1), nonce, c, s), at),
           ("proof_c = 0", enc(nym, nonce, 0, s), at), ("proof_s = 0", enc(nym, nonce, c, 0), at),
           ("proof_c >= r", enc(nym, nonce, c + Cv.r if c + Cv.r < 1 << 256 else (1 << 256) - 1, s), at),
           ("other issuer key", R.new_cred_request(other, r["sks"][7], nonce, 12345), at),
           ("Nym off the curve", enc((nym[0], (nym[1] + 1) % Cv.p), nonce, c, s), at),
           ("Nym = O", enc((0, 0), nonce, c, s), at),
           ("31-byte proof_c", enc(nym, nonce, OI.zr_bytes(c)[1:], s), at),
           ("33-byte proof_s", enc(nym, nonce, c, b"\0" + OI.zr_bytes(s)), at),
           ("31-byte nonce", enc(nym, nonce[1:], c, s), at),
           ("no proof_s", b"".join(OI.pb_bytes_field(q, v) for q, _, v in f if q != 4), at),
           ("truncated", req[:-1], at), ("empty", b"", at), ("NULL", None, at),
           ("attribute >= r", r["reqs"][8], [1, 2, Cv.r, 3]), ("NULL attributes", r["reqs"][9], None),
           ("honest last", r["reqs"][10], r["attrs"][10])]
    if s + Cv.r < 1 << 256:  # always on BN254; on FP256BN only for an s below 2^256 - r
        out.insert(9, ("proof_s + r", enc(nym, nonce, c, s + Cv.r), at))
    res = []
    for name, q, a in out:
        want = R.check_request(ipk, q)
        bad_attr = a is None or any(v >= Cv.r for v in a)
        res.append((name, q, a, want, R.BADKEY if bad_attr else want))
    return res


@pytest.mark.parametrize("tag", TAGS)
def test_verdicts(handles, tag):
    V, S = handles[tag]
    batch = verdict_batch(tag)
    want = {name: w for name, _, _, _, w in batch}
    # the restatement's verdicts are the ones the names say
    for name, w in want.items():
        exp = (R.OK if name.startswith("honest") or name == "proof_s + r" else
               R.BADKEY if "ttribute" in name else
               R.MALFORMED if name in ("Nym off the curve", "Nym = O", "31-byte proof_c", "33-byte proof_s",
                                       "31-byte nonce", "no proof_s", "truncated", "empty", "NULL") else R.INVALID)
        assert w == exp, name
    seed = 606
    creds, st = S.issue([q for _, q, _, _, _ in batch], [a for _, _, a, _, _ in batch], seed=seed)
    got = {name: int(s) for (name, _, _, _, _), s in zip(batch, st)}
    print(tag, got)
    assert got == want
    # rejected items: zeros and no length
    buf = S.last_buffer
    for j, (name, _, _, _, w) in enumerate(batch):
        assert (len(creds[j]) == 344) == (w == R.OK), name
        if w != R.OK:
            assert buf[344 * j:344 * (j + 1)] == bytes(344), name
    # the accepted items' bytes are those of a batch in which every other item is honest too
    honest_q, honest_a = batch[0][1], batch[0][2]
    all_good, st2 = S.issue([q if w == R.OK else honest_q for _, q, _, _, w in batch],
                            [a if w == R.OK else honest_a for _, _, a, _, w in batch], seed=seed)
    assert _ok(st2)
    for j, (name, _, _, _, w) in enumerate(batch):
        if w == R.OK:
            assert creds[j] == all_good[j], name
    # and they verify (proof_s + r among them: the same credential as for proof_s)
    sks = ref(tag)["sks"]
    sk_of = {"honest 0": sks[0], "honest 7": sks[7], "proof_s + r": sks[7], "honest last": sks[10]}
    good = [(creds[j], sk_of[name]) for j, (name, _, _, _, w) in enumerate(batch) if w == R.OK]
    assert _ok(V.verify_credentials([c for c, _ in good], [k for _, k in good]))


@pytest.mark.parametrize("tag", TAGS)
def test_request_verifier_agrees_with_the_issuer(handles, tag):
    V, _ = handles[tag]
    batch = verdict_batch(tag)
    st = V.verify_cred_requests([q for _, q, _, _, _ in batch])
    assert {name: int(s) for (name, _, _, _, _), s in zip(batch, st)} == {name: w for name, _, _, w, _ in batch}
    assert V.last_cred_request_kernel_ms()[1] > 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_request_generator_rejects_bad_secrets(handles, tag):
    V, _ = handles[tag]
    Cv = R.CURVES[tag][1]
    r = ref(tag)
    sks = [r["sks"][0], Cv.r, r["sks"][2], (1 << 256) - 1, r["sks"][4]]
    reqs, st = V.make_cred_requests(sks, r["nonces"][:5], seed=SEED_REQ)
    assert [int(s) for s in st] == [0, R.BADKEY, 0, R.BADKEY, 0]
    assert [reqs[j] for j in (0, 2, 4)] == [r["reqs"][j] for j in (0, 2, 4)] and reqs[1] == reqs[3] == b""
    assert V.last_request_buffer[172:344] == bytes(172)


# ------------------------------------------------- 6. API edges
def test_api_edges(handles):
    from fts_gpu import _lib as L
    V, S = handles["bn254"]
    r = ref("bn254")
    creds, st = S.issue([], [])
    assert creds == [] and len(st) == 0 and V.make_cred_requests([], [])[0] == []
    assert len(V.verify_cred_requests([])) == 0
    # a short stride: FTS_API_ESIZE with nothing written
    for call in (lambda: S.issue(r["reqs"][:2], r["attrs"][:2], stride=343),
                 lambda: V.make_cred_requests(r["sks"][:2], r["nonces"][:2], stride=171)):
        with pytest.raises(L.FtsError) as e:
            call()
        assert e.value.code == API_ESIZE
    st = np.full(2, -7, dtype=np.int32)
    buf = (C.c_uint8 * 700)(*([0xAA] * 700))
    ln = (C.c_uint32 * 2)(9, 9)
    items = (L.CredIssueItem * 2)()
    assert L.lib.fts_idemix_cred_issue_batch(S.h, 2, items, 1, buf, 343, ln, st.ctypes.data_as(C.POINTER(C.c_int32))) == API_ESIZE
    assert bytes(buf) == b"\xaa" * 700 and list(ln) == [9, 9] and list(st) == [-7, -7]
    assert L.lib.fts_idemix_cred_issue_batch(S.h, (1 << 22) + 1, items, 1, buf, 344, ln,
                                             st.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    # a wider stride: each credential at its own offset, the gap untouched
    creds, st = S.issue(r["reqs"][:3], r["attrs"][:3], seed=SEED_ISS, stride=400)
    assert _ok(st) and creds == r["creds"][:3] and S.last_buffer[344:400] == bytes(56)
    ms = S.last_timings()
    assert ms[0] > 0.0 and ms[1] > 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_two_threads_on_one_handle(handles, tag):
    V, S = handles[tag]
    r = ref(tag)
    n = 200
    out = [None] * 4

    def work(k):
        creds, st = S.issue(r["reqs"][:n], r["attrs"][:n], seed=SEED_ISS)
        reqs, st2 = V.make_cred_requests(r["sks"][:n], r["nonces"][:n], seed=SEED_REQ)
        out[k] = (creds, [int(s) for s in st], reqs, [int(s) for s in st2])
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for o in out:
        assert o == (r["creds"][:n], [0] * n, r["reqs"][:n], [0] * n)


def test_tile_edge(handles):
    """16,385 items on BN254 (one past a tile of 16,384): every credential verifies; the first
    item, the two at the edge and the last are byte-exact"""
    from fts_gpu import idemix as I
    cid, Cv, _ = R.CURVES["bn254"]
    isk, raw, ipk = key("bn254")
    n = 16385
    rng = random.Random(99)
    sks = [rng.randrange(1 << 248) for _ in range(n)]
    nonces = [rng.randbytes(32) for _ in range(n)]
    attrs = [[j, 2, 3, 4] for j in range(n)]
    V, S = handles["bn254"]
    reqs, st = V.make_cred_requests(sks, nonces, seed=SEED_REQ)
    assert _ok(st) and _ok(V.verify_cred_requests(reqs))
    creds, st = S.issue(reqs, attrs, seed=SEED_ISS)
    assert _ok(st) and _ok(V.verify_credentials(creds, sks))
    for j in (0, 16383, 16384):
        want = R.new_cred_request(ipk, sks[j], nonces[j], I.cred_issue_draws(cid, SEED_REQ, j)[2])
        assert reqs[j] == want, j
        E, Sd, _ = I.cred_issue_draws(cid, SEED_ISS, j)
        assert creds[j] == R.cred_proto(R.new_credential(ipk, isk, want, attrs[j], E, Sd)), j
