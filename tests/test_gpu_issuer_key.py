"""GPU: idemix issuer keys on the device, on both curves -- IssuerPublicKey.Check
(fts_idemix_ipk_check_batch) on the reference's four keys and on their mutations, verdict for
verdict against the restatement of tests/issuer_key_ref.py; NewIssuerKey
(fts_idemix_issuer_keygen_batch) byte-exact against tests/cred_issue_ref.py make_issuer_key at the
library's draws; and the whole chain from a generated key to verified identities.

Every case is a few keys: each kernel runs one lane per key."""
import functools
import random

import pytest

import cred_issue_ref as R
import issuer_key_ref as K
from oracle import idemix as OI, idemix_identity as ID

pytestmark = pytest.mark.gpu

TAGS = ["bn254", "fp256bn"]
API_EPP = -2
SEED = 7300


def _st(st):
    return [int(s) for s in st]


@functools.lru_cache(maxsize=None)
def cases(tag):
    """the honest key and its mutants with the restatement's verdicts, computed once"""
    ms = K.mutants(tag, K.golden(K.GOLDEN_KEYS[tag][0]))
    ref = [K.check(tag, raw) for _, raw, _ in ms]
    assert ref == [expect for _, _, expect in ms]
    return ms, ref


# ------------------------------------------------- 1. the check
@pytest.mark.parametrize("tag", TAGS)
def test_golden_keys_pass(tag):
    """the reference's keys of the curve in one call: FTS_OK, and the hash that comes back is each
    key's stored hash field"""
    from fts_gpu import idemix as I
    keys = [K.golden(name) for name in K.GOLDEN_KEYS[tag]]
    st, hs = I.check_issuer_keys(keys, R.CURVES[tag][0], return_hashes=True)
    assert _st(st) == [K.OK, K.OK]
    assert hs == [K.stored_hash(k) for k in keys]
    assert _st(I.check_issuer_keys(keys, R.CURVES[tag][0], raise_on_error=True)) == [0, 0]


@pytest.mark.parametrize("tag", TAGS)
def test_mutants_get_the_restatement_verdicts(tag):
    """one call holding the honest key and every mutant; then the same keys in another order
    (an item's defect does not reach its neighbours)"""
    from fts_gpu import idemix as I
    cid = R.CURVES[tag][0]
    ms, ref = cases(tag)
    names = [m[0] for m in ms]
    assert names[0] == "honest" and "empty" in names and ("proof_s+r" in names) == (tag == "bn254")
    keys = [m[1] for m in ms]
    got = _st(I.check_issuer_keys(keys, cid))
    assert got == ref, [(n, g, r) for n, g, r in zip(names, got, ref) if g != r]
    assert got[0] == K.OK
    if tag == "bn254":  # + r fits 32 bytes there: ProofS is used mod r
        assert got[names.index("proof_s+r")] == K.OK
    perm = list(range(len(keys)))
    random.Random(5).shuffle(perm)
    assert _st(I.check_issuer_keys([keys[p] for p in perm], cid)) == [ref[p] for p in perm]
    # a NULL item is malformed too
    assert _st(I.check_issuer_keys([None, keys[0]], cid)) == [K.MALFORMED, K.OK]
    with pytest.raises(I.IssuerKeyError) as e:
        I.check_issuer_keys([keys[0], keys[names.index("proof_s+1")]], cid, raise_on_error=True)
    assert (e.value.status, e.value.index) == (K.PROOF, 1)
    assert str(e.value) == "zero knowledge proof in public key invalid"


@pytest.mark.parametrize("tag", TAGS)
def test_wrong_curve_is_refused(tag):
    """a key of the other curve does not decode"""
    from fts_gpu import idemix as I
    other = "fp256bn" if tag == "bn254" else "bn254"
    assert _st(I.check_issuer_keys([K.golden(K.GOLDEN_KEYS[other][0])], R.CURVES[tag][0])) == [K.MALFORMED]


@pytest.mark.parametrize("tag", TAGS)
def test_lane_edges(tag):
    """65 keys, one past a wave and a block: the golden key and a ProofS + 1 mutant alternating"""
    from fts_gpu import idemix as I
    ms, _ = cases(tag)
    good, bad = ms[0][1], dict((m[0], m[1]) for m in ms)["proof_s+1"]
    st = _st(I.check_issuer_keys([good if i % 2 == 0 else bad for i in range(65)], R.CURVES[tag][0]))
    assert st == [K.OK if i % 2 == 0 else K.PROOF for i in range(65)]


# ------------------------------------------------- 2. key generation
@pytest.mark.parametrize("tag", TAGS)
def test_keygen_matches_the_restatement(tag):
    """n = 3 at a fixed seed: the ten draws of the debug hook replayed into make_issuer_key give
    the same IssuerPublicKey bytes and the same isk; each key passes the device's check and the
    restatement's; W = g2 isk by the oracle"""
    from fts_gpu import idemix as I
    cid, Cv, PC = R.CURVES[tag]
    got = I.generate_issuer_keys(3, cid, seed=SEED)
    assert len(got) == 3 and all(len(ipk) == I.FTS_IDEMIX_IPK_LEN == 843 for _, ipk in got)
    for i, (isk, ipk) in enumerate(got):
        rng = K.ReplayRng(I.keygen_draws(cid, SEED, i))
        want_isk, want = R.make_issuer_key(tag, rng)
        assert rng.used == 9  # the tenth value of the hook is the stream's next, not consumed
        assert isk == want_isk and ipk == want
        assert K.check(tag, ipk) == K.OK
        assert ID.parse_ecp2(PC, K.field(ipk, 5)) == PC.g2_mul(PC.g2_gen, isk)
        assert [v for f, _, v in K.fields(ipk) if f == 1] == list(K.NAMES)
    st, hs = I.check_issuer_keys([ipk for _, ipk in got], cid, return_hashes=True)
    assert _st(st) == [0, 0, 0] and hs == [K.stored_hash(ipk) for _, ipk in got]
    # item i depends on (seed + i) alone
    assert I.generate_issuer_keys(1, cid, seed=SEED + 2) == got[2:]
    assert len({isk for isk, _ in got}) == 3


@pytest.mark.parametrize("tag", TAGS)
def test_keygen_lane_edges(tag):
    """65 keys: the product kernels' lanes are laid out as product * n + key, so an n that is no
    multiple of 64 makes a wave straddle two products; every key passes the check"""
    from fts_gpu import idemix as I
    cid = R.CURVES[tag][0]
    got = I.generate_issuer_keys(65, cid, seed=SEED)
    assert got[:3] == I.generate_issuer_keys(3, cid, seed=SEED)
    assert _st(I.check_issuer_keys([ipk for _, ipk in got], cid)) == [0] * 65
    assert len({isk for isk, _ in got}) == 65


@pytest.mark.parametrize("tag", TAGS)
def test_secure_source(tag):
    from fts_gpu import idemix as I
    cid = R.CURVES[tag][0]
    a, b = I.generate_issuer_keys(1, cid)[0], I.generate_issuer_keys(1, cid)[0]
    assert a != b and a[0] != b[0]
    assert _st(I.check_issuer_keys([a[1], b[1]], cid)) == [0, 0]


def test_stride_and_sizes():
    from fts_gpu import idemix as I, _lib as L
    wide = I.generate_issuer_keys(2, 1, seed=SEED, stride=1024)
    assert wide == I.generate_issuer_keys(2, 1, seed=SEED)
    assert I.generate_issuer_keys(0, 1, seed=SEED) == []
    with pytest.raises(L.FtsError) as e:
        I.generate_issuer_keys(1, 1, seed=SEED, stride=842)
    assert e.value.code == -5
    with pytest.raises(L.FtsError) as e:
        I.check_issuer_keys([K.golden("bn254_tokengen")], 1, device=4096)
    assert e.value.code == -3
    assert len(I.check_issuer_keys([], 1)) == 0


# ------------------------------------------------- 3. the chain closes
@pytest.mark.parametrize("tag", TAGS)
def test_chain_from_a_generated_key(tag):
    """keygen -> check -> verifier handle -> issuer handle -> a credential request -> its
    credential -> verified -> two identities -> verified; isk + 1 is refused as today"""
    from fts_gpu import idemix as I, _lib as L
    cid, Cv, _ = R.CURVES[tag]
    (isk, ipk), = I.generate_issuer_keys(1, cid, seed=SEED + 40)
    assert _st(I.check_issuer_keys([ipk], cid)) == [0]
    V = I.IdentityVerifier(ipk, device=0, curve=cid)
    try:
        with pytest.raises(L.FtsError) as e:
            I.Issuer(V, (isk + 1) % Cv.r or 1)
        assert e.value.code == API_EPP
        S = I.Issuer(V, isk)
        try:
            rng = random.Random(77 + cid)
            sks, nonces = [rng.randrange(1, Cv.r)], [rng.randbytes(32)]
            attrs = [[rng.randrange(Cv.r) for _ in range(4)]]
            reqs, st = V.make_cred_requests(sks, nonces, seed=11)
            assert _st(st) == [0] and _st(V.verify_cred_requests(reqs)) == [0]
            creds, st = S.issue(reqs, attrs, seed=12)
            assert _st(st) == [0] and _st(V.verify_credentials(creds, sks)) == [0]
            cred = I.Credential(V, creds[0], sks[0])
            try:
                g = cred.generate(2, seed=13)
                assert _st(g.status) == [0, 0] and _st(V.verify_batch(g.ids)) == [0, 0]
            finally:
                cred.close()
        finally:
            S.close()
    finally:
        V.close()


def test_bn254_reference_secret():
    """bn254_tokengen/IssuerSecretKey with its public key: W = g2 isk, computed by the oracle
    only.  This test does not run the device's G2 product on the reference's secret: that
    product has no public entry of its own and key generation draws its own isk.  The device
    is asked only to accept the key (the check) and the secret (the issuer handle's G1 test);
    its g2 isk is compared with the oracle's in test_keygen_matches_the_restatement"""
    from fts_gpu import idemix as I
    isk, raw = R.tokengen()
    PC = R.PR.BN254
    assert ID.parse_ecp2(PC, K.field(raw, 5)) == PC.g2_mul(PC.g2_gen, isk)
    assert _st(I.check_issuer_keys([raw], 1)) == [0]
    V = I.IdentityVerifier(raw, device=0, curve=1)
    try:
        I.Issuer(V, isk).close()
    finally:
        V.close()
