"""GPU: idemix owner identities generated on the device (fts_idemix_cred,
fts_idemix_identity_generate_batch) on both curves, from the reference's own credentials
(tests/golden/idemix): bytes against the oracle's signer at the library's draws, the
library's verifier, auditor and nym signer on the results, seeds, fixed audit randoms, the
credential and argument checks, threads, and a handle beside a live verifier.

The oracle positions are few: oracle/idemix.py on FP256BN costs 0.1-0.2 s per scalar
product, some twenty per identity."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import idemix_audit_ref as REF
import idgen_common as G
from oracle import idemix as OI, idemix_identity as ID

pytestmark = pytest.mark.gpu

N = 130  # two full waves and a ragged tail
SEED = 4242
POSITIONS = (0, 1, 63, 64, 127, 129)
API_EINVAL, API_EPP, API_ESIZE = -1, -2, -5


@pytest.fixture(scope="module", params=["bn254", "fp256bn"])
def case(request):
    from fts_gpu import idemix as I
    tag = request.param
    _, cid, Cv, PC = G.CURVES[tag]
    ipk, cred, W = G.oracle_key(tag)
    ver = I.IdentityVerifier(G.raw(tag, "IssuerPublicKey"), device=0, curve=cid)
    cred_raw, sk, cri = I.parse_signer_config(G.raw(tag, "SignerConfig"))
    dev = I.Credential(ver, cred_raw, sk)  # no CRI: epoch 0 and the generator, as the oracle's sign
    eid, rh = REF.signer_strings(G.raw(tag, "SignerConfig"))
    c = {"tag": tag, "cid": cid, "C": Cv, "PC": PC, "ipk": ipk, "cred": cred, "W": W, "ver": ver, "dev": dev,
         "cred_raw": cred_raw, "sk": sk, "cri": cri, "eid": eid, "rh": rh, "batch": dev.generate(N, seed=SEED)}
    yield c
    dev.close()
    ver.close()


def _proof(c, identity):
    f = OI.pb_fields(identity)
    return ID.decode_signature(OI._pb_bytes(f, 4), c["C"])


def _z32(v):
    return v.to_bytes(32, "big")


# ------------------------------------------------------------- the oracle
def test_bytes_equal_the_oracle(case):
    from fts_gpu import idemix as I
    c, b = case, case["batch"]
    assert not b.status.any() and len(b) == N
    assert c["dev"].identity_len == (1113 if c["tag"] == "bn254" else 1114)
    assert all(len(x) == c["dev"].identity_len for x in b.ids)
    for i in POSITIONS:
        d = c["dev"].draws(SEED, i)
        assert b.ids[i] == G.oracle_identity(c["tag"], c["ipk"], c["cred"], d), i
        assert (b.rnym[i], b.r_eid[i], b.r_rh[i]) == (_z32(d[0]), _z32(d[14]), _z32(d[15])), i
    for i in (0, 129):  # the oracle's own verifier, pairing included
        ID.verify_identity(c["ipk"], c["PC"], c["W"], b.ids[i])
    assert not c["ver"].verify_batch(b.ids).any()
    eids, rhs = [c["eid"]] * N, [c["rh"]] * N
    assert not c["ver"].audit_match_batch(b.ids, eids, b.r_eid, rhs, b.r_rh).any()
    eids[77] = c["eid"] + b"x"
    st = c["ver"].audit_match_batch(b.ids, eids, b.r_eid, rhs, b.r_rh)
    assert [int(s) for s in st] == [I.FTS_E_AUDIT_EID_MISMATCH if i == 77 else 0 for i in range(N)]
    t = c["dev"].last_timings()
    assert t[0] > 0 and t[1] > 0


def test_epoch_and_key_come_from_the_cri(case):
    """the fixture's own revocation information (BN254: epoch 1) instead of none"""
    from fts_gpu import idemix as I
    c = case
    epoch = dict((k, v) for k, wt, v in OI.pb_fields(c["cri"]) if wt == 0).get(1, 0)
    dev = I.Credential(c["ver"], c["cred_raw"], c["sk"], c["cri"])
    try:
        g = dev.generate(3, seed=SEED)
        assert not g.status.any()
        assert g.ids[2] == G.oracle_identity(c["tag"], c["ipk"], c["cred"], dev.draws(SEED, 2), epoch=epoch)
        assert (g.ids == c["batch"].ids[:3]) == (epoch == 0)
        assert not c["ver"].verify_batch(g.ids).any()
    finally:
        dev.close()


# ----------------------------------------------------------------- owners
def test_generated_identities_sign_as_owners(case):
    from fts_gpu import idemix as I
    c, b = case, case["batch"]
    key = I.IssuerKey(G.raw(c["tag"], "IssuerPublicKey"), device=0, curve=c["cid"])
    try:
        idx = [0, 1, 64, 129]
        nyms = [I.identity_nym(b.ids[i]) for i in idx]
        msgs = [b"request %d" % i for i in idx]
        sigs, st = key.sign_batch([c["sk"]] * 4, [b.rnym[i] for i in idx], nyms, msgs, seed=5, return_status=True)
        assert not st.any()
        assert not key.verify_batch(nyms, sigs, msgs).any()
        assert all(int(s) == I.FTS_E_NYM_INVALID for s in key.verify_batch(nyms, sigs, msgs[1:] + msgs[:1]))
    finally:
        key.close()


# ------------------------------------------------------------------ seeds
def test_seeds(case):
    c, b, dev = case, case["batch"], case["dev"]
    again = dev.generate(N, seed=SEED)
    assert again.ids == b.ids and again.rnym == b.rnym and again.r_eid == b.r_eid and again.r_rh == b.r_rh
    for i in (0, 1, 63, 64, 129):
        one = dev.generate(1, seed=SEED + i)
        assert (one.ids[0], one.rnym[0], one.r_eid[0], one.r_rh[0]) == (b.ids[i], b.rnym[i], b.r_eid[i], b.r_rh[i]), i
    other = dev.generate(N, seed=SEED + 1000)

    def nyms_aprimes(g):
        from fts_gpu import idemix as I
        return [I.identity_nym(x) for x in g.ids], [_proof(c, x)["APrime"] for x in g.ids]
    na, aa = nyms_aprimes(b)
    nb, ab = nyms_aprimes(other)
    assert len(set(na + nb)) == 2 * N and len(set(aa + ab)) == 2 * N
    o1, o2 = dev.generate(N), dev.generate(N)  # the OS source
    n1, n2 = nyms_aprimes(o1)[0], nyms_aprimes(o2)[0]
    assert len(set(n1 + n2)) == 2 * N
    assert not c["ver"].verify_batch(o1.ids + o2.ids + other.ids).any()


# ----------------------------------------------------- fixed audit randoms
def test_fixed_audit_randoms(case):
    from fts_gpu import idemix as I
    c, b, dev = case, case["batch"], case["dev"]
    r = c["C"].r
    re_, rr = int.from_bytes(b.r_eid[5], "big"), int.from_bytes(b.r_rh[9], "big")
    g = dev.generate(N, seed=SEED, r_eid=re_, r_rh=rr)
    assert not g.status.any()
    assert g.rnym == b.rnym  # the draws at the other positions did not move
    assert set(g.r_eid) == {_z32(re_)} and set(g.r_rh) == {_z32(rr)}
    pr = [_proof(c, x) for x in g.ids]
    assert {p["EidNym"] for p in pr} == {_proof(c, b.ids[5])["EidNym"]}
    assert {p["RhNym"] for p in pr} == {_proof(c, b.ids[9])["RhNym"]}
    assert len({I.identity_nym(x) for x in g.ids}) == N
    assert g.ids[5] != b.ids[5] and [p["APrime"] for p in pr] == [_proof(c, x)["APrime"] for x in b.ids]
    assert not c["ver"].verify_batch(g.ids).any()
    assert not c["ver"].audit_match_batch(g.ids, [c["eid"]] * N, g.r_eid, [c["rh"]] * N, g.r_rh).any()
    # an in-value of r and one of 2^256 - 1 between valid items
    eids = [int.from_bytes(x, "big") for x in b.r_eid[:7]]
    rhs = [int.from_bytes(x, "big") for x in b.r_rh[:7]]
    eids[2], rhs[4] = r, (1 << 256) - 1
    h = dev.generate(7, seed=SEED, r_eid=eids, r_rh=rhs)
    assert [int(s) for s in h.status] == [I.FTS_E_SIGN_BADKEY if i in (2, 4) else 0 for i in range(7)]
    for i in range(7):
        if i in (2, 4):
            assert h.ids[i] == b"" and h.rnym[i] == h.r_eid[i] == h.r_rh[i] == bytes(32)
        else:  # the drawn values handed back in: the batch's own identities
            assert (h.ids[i], h.rnym[i], h.r_eid[i], h.r_rh[i]) == (b.ids[i], b.rnym[i], b.r_eid[i], b.r_rh[i])
    # the rejected items' bytes are zero in the caller's buffer too
    st, ids = _raw_generate(dev, 7, SEED, r_eid=b"".join(_z32(x) for x in eids), fill=0xAA)
    ln = dev.identity_len
    assert st == 0 and ids[2 * ln:3 * ln] == bytes(ln) and ids[3 * ln:4 * ln] == b.ids[3]


def _raw_generate(dev, n, seed, r_eid=None, stride=None, fill=0):
    """the C entry point on a caller's buffer pre-filled with `fill` -> (API code, buffer)"""
    from fts_gpu import _lib as L
    stride = dev.identity_len if stride is None else stride
    ids = np.full(max(1, n * max(stride, 1)), fill, dtype=np.uint8)
    lens = np.zeros(max(1, n), dtype=np.uint32)
    rn, re_, rr = (np.zeros(max(1, 32 * n), dtype=np.uint8) for _ in range(3))
    st = np.zeros(max(1, n), dtype=np.int32)
    keep = None if r_eid is None else np.frombuffer(r_eid, dtype=np.uint8)
    code = L.lib.fts_idemix_identity_generate_batch(dev.h, n, seed, None if keep is None else keep.ctypes.data, None,
                                                    ids.ctypes.data, stride, lens.ctypes.data, rn.ctypes.data,
                                                    re_.ctypes.data, rr.ctypes.data,
                                                    st.ctypes.data_as(C.POINTER(C.c_int32)))
    return code, ids.tobytes()


# ------------------------------------------------------ credential checks
def _cred_proto(A, B, E, S, attrs):
    out = OI.pb_bytes_field(1, ID.ecp(A)) + OI.pb_bytes_field(2, ID.ecp(B)) + \
        OI.pb_bytes_field(3, OI.zr_bytes(E)) + OI.pb_bytes_field(4, OI.zr_bytes(S))
    return out + b"".join(OI.pb_bytes_field(5, OI.zr_bytes(a)) for a in attrs)


def test_credential_checks(case):
    from fts_gpu import idemix as I, _lib as L
    c, k = case, case["cred"]
    Cv = c["C"]
    A, B, E, S, attrs, sk = k["A"], k["B"], k["E"], k["S"], k["attrs"], k["sk"]
    assert _cred_proto(A, B, E, S, attrs) == c["cred_raw"]
    bad = {
        "wrong sk": (_cred_proto(A, B, E, S, attrs), (sk + 1) % Cv.r),
        "wrong S": (_cred_proto(A, B, E, (S + 1) % Cv.r, attrs), sk),
        "wrong attribute": (_cred_proto(A, B, E, S, attrs[:3] + [(attrs[3] + 1) % Cv.r]), sk),
        "three attributes": (_cred_proto(A, B, E, S, attrs[:3]), sk),
        "A off the curve": (_cred_proto((A[0], (A[1] + 1) % Cv.p), B, E, S, attrs), sk),
        "B off the curve": (_cred_proto(A, (B[0], (B[1] + 1) % Cv.p), E, S, attrs), sk),
        "A = O": (_cred_proto((0, 0), B, E, S, attrs), sk),
        "E = r": (_cred_proto(A, B, Cv.r, S, attrs), sk),
        "sk = r": (_cred_proto(A, B, E, S, attrs), Cv.r),
    }
    for name, (raw, s) in bad.items():
        with pytest.raises(L.FtsError) as e:
            I.Credential(c["ver"], raw, s)
        assert e.value.code == API_EPP, name
    # a forged A that passes every check made here: its identities fail the verifier's pairing
    forged = I.Credential(c["ver"], _cred_proto(Cv.mul(A, 2), B, E, S, attrs), sk)
    try:
        g = forged.generate(2, seed=1)
        assert [int(s) for s in c["ver"].verify_batch(g.ids)] == [I.FTS_E_ID_PAIRING] * 2
    finally:
        forged.close()


def test_argument_checks(case):
    from fts_gpu import idemix as I, _lib as L
    c, dev = case, case["dev"]
    with pytest.raises(L.FtsError) as e:  # a revocation algorithm set
        I.Credential(c["ver"], c["cred_raw"], c["sk"], c["cri"] + ID._varint_field(4, 1))
    assert e.value.code == API_EPP
    with pytest.raises(L.FtsError) as e:
        I.Credential(c["ver"], b"", c["sk"])
    assert e.value.code == API_EINVAL
    ln = dev.identity_len
    code, buf = _raw_generate(dev, 3, SEED, stride=ln - 1, fill=0x5C)
    assert code == API_ESIZE and buf == b"\x5c" * (3 * (ln - 1))
    code, buf = _raw_generate(dev, 0, SEED, fill=0x5C)
    assert code == 0 and buf == b"\x5c"
    assert len(dev.generate(0, seed=1)) == 0
    assert L.lib.fts_idemix_identity_generate_batch(dev.h, (1 << 22) + 1, 1, None, None, None, ln, None, None, None,
                                                    None, None) == API_EINVAL
    # a wider stride: the identities land at its multiples, the gaps are untouched
    code, buf = _raw_generate(dev, 2, SEED, stride=ln + 7, fill=0x5C)
    assert code == 0 and buf[:ln] == c["batch"].ids[0] and buf[ln:ln + 7] == b"\x5c" * 7
    assert buf[ln + 7:2 * ln + 7] == c["batch"].ids[1]


# ---------------------------------------------------------------- threads
def test_four_threads_generate_and_verify(case):
    c = case
    res = [None] * 4

    def work(t):
        try:
            g = c["dev"].generate(N, seed=9000 + 1000 * t)
            ok = not g.status.any() and not c["ver"].verify_batch(g.ids).any()
            res[t] = bool(ok) and g.ids[0] == c["dev"].generate(1, seed=9000 + 1000 * t).ids[0]
        except Exception as e:  # reported by the assertion below
            res[t] = e
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert res == [True] * 4


# ------------------------------------------------------------ coexistence
def test_handle_beside_a_live_verifier(case):
    from fts_gpu import idemix as I
    c = case
    with open(os.path.join(G.GOLD, "idemix_identity_golden.json")) as f:
        cases = json.load(f)[c["tag"]]["cases"]
    ids = [bytes.fromhex(x["identity"]) for x in cases]
    want = [x["error"] for x in cases]
    assert [I.message(int(s)) for s in c["ver"].verify_batch(ids)] == want
    other = I.Credential.from_signer_config(c["ver"], G.raw(c["tag"], "SignerConfig"))
    g = other.generate(5, seed=3)
    assert [I.message(int(s)) for s in c["ver"].verify_batch(ids + g.ids)] == want + [None] * 5
    other.close()
    assert [I.message(int(s)) for s in c["ver"].verify_batch(ids)] == want
    assert c["dev"].generate(N, seed=SEED).ids == c["batch"].ids


# ------------------------------------------------------------------ tiles
def test_call_across_tiles(case):
    """a call above 16,384 identities runs in tiles: the items on both sides of the boundary
    and the last one equal the one-item calls at their seeds, and every identity verifies"""
    c, dev = case, case["dev"]
    n = 16384 + 130
    g = dev.generate(n, seed=SEED)
    assert not g.status.any() and g.ids[:N] == c["batch"].ids
    for i in (16383, 16384, 16385, n - 1):
        one = dev.generate(1, seed=SEED + i)
        assert (one.ids[0], one.rnym[0], one.r_eid[0], one.r_rh[0]) == (g.ids[i], g.rnym[i], g.r_eid[i], g.r_rh[i]), i
    assert len({x[:70] for x in g.ids}) == n  # the nym public keys differ
    assert not c["ver"].verify_batch(g.ids).any()
