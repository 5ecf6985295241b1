"""GPU: idemix credentials verified on the device (fts_idemix_cred_verify_batch), pairing
equation included, on both curves: the reference's credentials (tests/golden/idemix) under
their own and another issuer's key, the order of the verdicts over every tampering that
fts_idemix_cred_create rejects plus the ones it cannot see (a forged A, a wrong E), agreement
with fts_idemix_cred_create, the edges of the groups of 256 of the randomised pairing check,
E A - B = O, the per-item mode, the identity calls' bookkeeping, two threads on one handle,
and the edge of a tile of 16,384.

BN254 credentials are issued here with the oracle curve under bn254_tokengen, whose
IssuerSecretKey the fixtures hold.  The oracle's pairing confirms a handful of verdicts; every
other expected verdict follows by construction."""
import functools
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import PKG

import cred_common as K
from oracle import idemix_identity as ID

pytestmark = pytest.mark.gpu

API_EINVAL, API_EPP = -1, -2
OK, MALFORMED, BVAL, PAIRING = 0, 36, 37, 38


def _sk(k):
    return k["sk"].to_bytes(32, "big")


@pytest.fixture(scope="module")
def handles():
    from fts_gpu import idemix as I
    hs = {name: I.IdentityVerifier(K.raw(name, "IssuerPublicKey"), device=0, curve=cid)
          for name, (cid, _, _) in K.ISSUERS.items()}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def issued():
    """8 honest BN254 credentials under bn254_tokengen, their protos and 2 A forgeries"""
    rng = random.Random(77)
    ks = [K.issue_bn254(rng) for _ in range(8)]
    C = K.ISSUERS["bn254_tokengen"][1]
    return {"k": ks, "good": [(K.cred_proto(k), _sk(k)) for k in ks],
            "forged": [(K.cred_proto(k, A=C.mul(k["A"], 2)), _sk(k)) for k in ks]}


@functools.lru_cache(maxsize=None)
def _verdict_batch(issuer):
    """[(name, cred or None, sk or None, expected verdict)] around the issuer's reference credential"""
    C = K.ISSUERS[issuer][1]
    k = K.signer(issuer)
    sk, r, p = k["sk"], C.r, C.p
    A, B = k["A"], k["B"]
    z = lambda v: v.to_bytes(32, "big")  # noqa: E731
    return [
        ("honest", K.cred_proto(k), z(sk), OK),
        ("wrong sk", K.cred_proto(k), z((sk + 1) % r), BVAL),
        ("wrong S", K.cred_proto(k, S=(k["S"] + 1) % r), z(sk), BVAL),
        ("wrong attribute", K.cred_proto(k, attrs=k["attrs"][:3] + [(k["attrs"][3] + 1) % r]), z(sk), BVAL),
        ("three attributes", K.cred_proto(k, attrs=k["attrs"][:3]), z(sk), MALFORMED),
        ("A off the curve", K.cred_proto(k, A=(A[0], (A[1] + 1) % p)), z(sk), MALFORMED),
        ("B off the curve", K.cred_proto(k, B=(B[0], (B[1] + 1) % p)), z(sk), MALFORMED),
        ("A = O", K.cred_proto(k, A=(0, 0)), z(sk), MALFORMED),
        ("E = r", K.cred_proto(k, E=r), z(sk), MALFORMED),
        ("sk = r", K.cred_proto(k), z(r), MALFORMED),
        ("NULL sk32", K.cred_proto(k), None, MALFORMED),
        ("empty cred", b"", z(sk), MALFORMED),
        ("A = 2 A", K.cred_proto(k, A=C.mul(A, 2)), z(sk), PAIRING),
        ("wrong E", K.cred_proto(k, E=(k["E"] + 1) % r), z(sk), PAIRING),
        ("wrong S and A = 2 A", K.cred_proto(k, S=(k["S"] + 1) % r, A=C.mul(A, 2)), z(sk), BVAL),
    ]


BATCH_ISSUER = {"bn254": "bn254_charlie", "fp256bn": "fp256bn_validator"}


# ------------------------------------------------- 1. reference credentials
def test_reference_credentials(handles):
    bn, fb, fb2 = K.signer("bn254_charlie"), K.signer("fp256bn_validator"), K.signer("fp256bn_validator", "SignerConfig2")
    assert [int(s) for s in handles["bn254_charlie"].verify_credentials([K.cred_proto(bn)], [_sk(bn)])] == [OK]
    two = ([K.cred_proto(fb), K.cred_proto(fb2)], [_sk(fb), _sk(fb2)])
    assert [int(s) for s in handles["fp256bn_validator"].verify_credentials(*two)] == [OK, OK]
    # under another issuer of the curve: other bases, so B does not match
    assert [int(s) for s in handles["bn254_tokengen"].verify_credentials([K.cred_proto(bn)], [_sk(bn)])] == [BVAL]
    assert [int(s) for s in handles["fp256bn_crypto"].verify_credentials(*two)] == [BVAL, BVAL]
    # the signer config's own proto, as parse_signer_config hands it to fts_idemix_cred_create
    from fts_gpu import idemix as I
    cred, sk, _ = I.parse_signer_config(K.raw("fp256bn_validator", "SignerConfig2"))
    handles["fp256bn_validator"].VerifyCredential(cred, sk)
    with pytest.raises(I.IdentityError) as e:
        handles["fp256bn_crypto"].VerifyCredential(cred, sk)
    assert e.value.status == BVAL and str(e.value) == I.message(BVAL)


# --------------------------------------------------------- 2. verdict order
@pytest.mark.parametrize("tag", ["bn254", "fp256bn"])
def test_verdict_order(handles, tag):
    from fts_gpu import idemix as I
    issuer = BATCH_ISSUER[tag]
    V = handles[issuer]
    batch = _verdict_batch(issuer)
    st = V.verify_credentials([c for _, c, _, _ in batch], [s for _, _, s, _ in batch])
    got = {name: int(s) for (name, _, _, _), s in zip(batch, st)}
    print(tag, got)
    assert got == {name: e for name, _, _, e in batch}
    # the one group holds failing equations: its items still FTS_OK after the B check (the honest
    # one, 2 A and the wrong E) are paired one by one, the others never reach the pairing stage
    assert V.last_cred_stats() == (1, 3)
    # the oracle on the three verdicts the pairing decides
    _, C, PC = K.ISSUERS[issuer]
    k = K.signer(issuer)
    ipk, W = K.oracle_ipk(issuer)
    assert ID.credential_b(ipk, k) == k["B"]
    assert ID.credential_pairing_ok(PC, W, k) is True
    assert ID.credential_pairing_ok(PC, W, dict(k, A=C.mul(k["A"], 2))) is False
    assert ID.credential_pairing_ok(PC, W, dict(k, E=(k["E"] + 1) % C.r)) is False
    with pytest.raises(I.IdentityError) as e:
        V.VerifyCredential(batch[12][1], batch[12][2])
    assert str(e.value) == "credential is not cryptographically valid" and e.value.status == PAIRING


# ------------------------------------- 3. consistency with fts_idemix_cred_create
@pytest.mark.parametrize("tag", ["bn254", "fp256bn"])
def test_consistent_with_cred_create(handles, tag):
    from fts_gpu import idemix as I, _lib as L
    issuer = BATCH_ISSUER[tag]
    V = handles[issuer]
    batch = [b for b in _verdict_batch(issuer) if b[1] is not None and b[2] is not None]
    st = V.verify_credentials([c for _, c, _, _ in batch], [s for _, _, s, _ in batch])
    for (name, cred, sk, _), s in zip(batch, st):
        code = 0
        try:
            I.Credential(V, cred, sk).close()
        except L.FtsError as e:
            code = e.code
        if not cred:  # an empty proto never reaches create's checks: its argument check answers
            assert code == API_EINVAL and int(s) == MALFORMED, name
            continue
        assert (code == API_EPP) == (int(s) in (MALFORMED, BVAL)), (name, code, int(s))
        assert code in (0, API_EPP), (name, code)
        if name in ("A = 2 A", "wrong E"):
            assert code == 0 and int(s) == PAIRING, name


# ------------------------------------------------------------ 4. group edges
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_group_edges_honest(handles, issued, n):
    V = handles["bn254_tokengen"]
    items = [issued["good"][i % 8] for i in range(n)]
    st = V.verify_credentials([c for c, _ in items], [s for _, s in items])
    assert not st.any()
    assert V.last_cred_stats() == ((n + 255) // 256, 0)
    t = V.last_cred_kernel_ms()
    assert t[0] > 0 and t[1] > 0


@pytest.mark.parametrize("bad,paired", [((0, 255, 256, 512), 513), ((300,), 256)])
def test_group_edges_forged(handles, issued, bad, paired):
    V = handles["bn254_tokengen"]
    items = [issued["forged" if i in bad else "good"][i % 8] for i in range(513)]
    st = V.verify_credentials([c for c, _ in items], [s for _, s in items])
    assert [i for i in range(513) if st[i]] == list(bad)
    assert {int(st[i]) for i in bad} == {PAIRING}
    assert V.last_cred_stats() == (3, paired)


def test_empty_batch(handles):
    from fts_gpu import _lib as L
    V = handles["bn254_tokengen"]
    assert L.lib.fts_idemix_cred_verify_batch(V.h, 0, None, None) == 0
    assert len(V.verify_credentials([], [])) == 0
    assert L.lib.fts_idemix_cred_verify_batch(V.h, 1, None, None) == API_EINVAL
    assert L.lib.fts_idemix_cred_verify_batch(V.h, (1 << 22) + 1, None, None) == API_EINVAL


# ------------------------------------------------------------------ 5. T = O
def test_t_is_the_identity(handles):
    """A = B E^-1: E A - B = O, which the pairing stage reads as e(g2, O) = 1; e(W, A) != 1"""
    rng = random.Random(5)
    C = K.ISSUERS["bn254_tokengen"][1]
    V = handles["bn254_tokengen"]
    k = K.issue_bn254(rng, plain_inverse=True)
    assert C.add(C.mul(k["A"], k["E"]), C.neg(k["B"])) is None
    good = K.issue_bn254(rng)
    st = V.verify_credentials([K.cred_proto(k), K.cred_proto(good), K.cred_proto(k)], [_sk(k), _sk(good), _sk(k)])
    assert [int(s) for s in st] == [PAIRING, OK, PAIRING]
    assert [int(s) for s in V.verify_credentials([K.cred_proto(k)], [_sk(k)])] == [PAIRING]


# ---------------------------------------------------------- 6. per-item mode
_CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from fts_gpu import idemix as I
d = json.load(sys.stdin)
V = I.IdentityVerifier(bytes.fromhex(d["ipk"]), device=0, curve=1)
un = lambda x: None if x is None else bytes.fromhex(x)
st = V.verify_credentials([un(c) for c, _ in d["items"]], [un(s) for _, s in d["items"]])
print(json.dumps({"st": [int(s) for s in st], "stats": V.last_cred_stats()}))
V.close()
"""


def test_per_item_mode_in_a_child_process(handles):
    batch = _verdict_batch("bn254_charlie")
    hx = lambda x: None if x is None else x.hex()  # noqa: E731
    doc = {"ipk": K.raw("bn254_charlie", "IssuerPublicKey").hex(), "items": [(hx(c), hx(s)) for _, c, s, _ in batch]}
    env = dict(os.environ, FTS_IDV_BATCH="0")
    p = subprocess.run([sys.executable, "-c", _CHILD, PKG, os.path.dirname(PKG)], input=json.dumps(doc), env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().split("\n")[-1])
    assert out["st"] == [e for _, _, _, e in batch]
    assert out["stats"] == [0, len(batch)]


# ------------------------------------------------- 7. identity bookkeeping
@pytest.fixture(scope="module")
def identities(handles):
    """130 owner identities generated from bn254_charlie's signer config"""
    from fts_gpu import idemix as I
    V = handles["bn254_charlie"]
    dev = I.Credential.from_signer_config(V, K.raw("bn254_charlie", "SignerConfig"), with_cri=False)
    try:
        g = dev.generate(130, seed=31)
    finally:
        dev.close()
    assert not g.status.any()
    ids = list(g.ids)
    ids[7] = ids[7][:-1]  # a malformed one among them
    return ids


def _creds_130():
    k = K.signer("bn254_charlie")
    C = K.ISSUERS["bn254_charlie"][1]
    good, forged = (K.cred_proto(k), _sk(k)), (K.cred_proto(k, A=C.mul(k["A"], 2)), _sk(k))
    return [forged if i in (3, 129) else good for i in range(130)]


def test_identity_bookkeeping_untouched(handles, identities):
    V = handles["bn254_charlie"]
    st_id = V.verify_batch(identities)
    stats, ms = V.last_pairing_stats(), V.last_kernel_ms()
    assert st_id[7] != 0 and not np.delete(st_id, 7).any() and stats == (1, 0)
    items = _creds_130()
    st = V.verify_credentials([c for c, _ in items], [s for _, s in items])
    assert [i for i in range(130) if st[i]] == [3, 129] and V.last_cred_stats() == (1, 130)
    assert V.last_pairing_stats() == stats and V.last_kernel_ms() == ms
    assert (V.verify_batch(identities) == st_id).all()
    assert V.last_cred_stats() == (1, 130)


# ------------------------------------------------------------- 8. two threads
def test_two_threads_on_one_handle(handles, identities):
    V = handles["bn254_charlie"]
    items = _creds_130()
    creds, sks = [c for c, _ in items], [s for _, s in items]
    serial = (V.verify_batch(identities), V.verify_credentials(creds, sks))
    res = {}

    def run(name, fn):
        try:
            res[name] = [fn() for _ in range(3)]
        except Exception as e:  # reported by the assertions below
            res[name] = e
    th = [threading.Thread(target=run, args=("id", lambda: V.verify_batch(identities))),
          threading.Thread(target=run, args=("cred", lambda: V.verify_credentials(creds, sks)))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert isinstance(res["id"], list) and isinstance(res["cred"], list), res
    assert all((r == serial[0]).all() for r in res["id"])
    assert all((r == serial[1]).all() for r in res["cred"])


# ---------------------------------------------------------------- 9. tile edge
def test_tile_edge(handles, issued):
    V = handles["bn254_tokengen"]
    n = 16385
    items = [issued["good"][i % 8] for i in range(n - 1)] + [issued["forged"][0]]
    st = V.verify_credentials([c for c, _ in items], [s for _, s in items])
    assert [int(i) for i in np.nonzero(st)[0]] == [n - 1] and int(st[n - 1]) == PAIRING
    assert V.last_cred_stats() == (64 + 1, 1)
