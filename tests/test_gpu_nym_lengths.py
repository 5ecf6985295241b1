"""GPU: nym signatures over every padding position of the hashed stream, on both
curves.  One batch of 192 items with message lengths 0..191: the stream is the
164-byte (BN254) or 166-byte (FP256BN) prefix and the message, so every residue of
its length mod 64 occurs three times, the 55/56 edge (a further block for the bit
length) and the 63/0 edge among them.  The device signs with a fixed seed; the oracle
(oracle/idemix.py nym_verify) must accept every signature and reject the message with
its last byte flipped, and the device verifier must say the same, in one launch and
in three tiles of 64."""
import json
import os
import random

import pytest

from conftest import GOLDEN

from oracle import idemix as O

pytestmark = pytest.mark.gpu

CURVES = {"bn254": 1, "fp256bn": 0}
PREFIX = {"bn254": 164, "fp256bn": 166}
N = 192

with open(os.path.join(GOLDEN, "idemix_golden.json")) as f:
    GOLD = json.load(f)


def _flip(m):
    return m[:-1] + bytes([m[-1] ^ 0x01])


@pytest.fixture(scope="module", params=["bn254", "fp256bn"])
def case(request):
    """the handle, the oracle's key, 192 seeded items (four pseudonyms in turn) and the
    device's signatures of them"""
    from fts_gpu import idemix as I
    name = request.param
    C = O.CURVES[CURVES[name]]
    raw = bytes.fromhex(GOLD[name]["ipk"])
    ipk = O.parse_ipk(raw, C)
    rng = random.Random(1920 + CURVES[name])
    keys = [(rng.randrange(C.r), rng.randrange(C.r)) for _ in range(4)]
    knym = [O.nym_bytes(ipk, O.make_nym(ipk, a, b)) for a, b in keys]
    sks = [keys[i % 4][0] for i in range(N)]
    rns = [keys[i % 4][1] for i in range(N)]
    nyms = [knym[i % 4] for i in range(N)]
    msgs = [rng.randbytes(ln) for ln in range(N)]
    dev = I.IssuerKey(raw, device=0, curve=CURVES[name])
    sigs, st = dev.sign_batch(sks, rns, nyms, msgs, seed=192, return_status=True)
    assert not st.any() and all(len(s) == 136 for s in sigs)
    yield {"name": name, "raw": raw, "ipk": ipk, "dev": dev, "nyms": nyms, "msgs": msgs, "sigs": sigs}
    dev.close()


def test_lengths_cover_every_padding_position(case):
    res = [(PREFIX[case["name"]] + len(m)) % 64 for m in case["msgs"]]
    assert all(res.count(r) == 3 for r in range(64))


def test_oracle_accepts_each_and_rejects_the_flipped_message(case):
    c = case
    for nym, m, sig in zip(c["nyms"], c["msgs"], c["sigs"]):
        O.nym_verify(c["ipk"], nym, sig, m)
        if m:
            with pytest.raises(O.NymError):
                O.nym_verify(c["ipk"], nym, sig, _flip(m))


def _device_verdicts(I, dev, c):
    st = dev.verify_batch(c["nyms"], c["sigs"], c["msgs"])
    assert [int(s) for s in st] == [I.FTS_OK] * N
    st = dev.verify_batch(c["nyms"][1:], c["sigs"][1:], [_flip(m) for m in c["msgs"][1:]])
    assert [int(s) for s in st] == [I.FTS_E_NYM_INVALID] * (N - 1)


def test_device_verifier_agrees(case):
    from fts_gpu import idemix as I
    _device_verdicts(I, case["dev"], case)


def test_device_verifier_agrees_in_three_tiles(case):
    """a fresh handle built with FTS_NYM_TILE=64 (tests/test_idemix.py
    test_launch_tiling_gives_same_verdicts): 192 = three launches"""
    from fts_gpu import idemix as I
    old = os.environ.get("FTS_NYM_TILE")
    os.environ["FTS_NYM_TILE"] = "64"
    try:
        k = I.IssuerKey(case["raw"], device=0, curve=CURVES[case["name"]])
    finally:
        if old is None:
            del os.environ["FTS_NYM_TILE"]
        else:
            os.environ["FTS_NYM_TILE"] = old
    try:
        _device_verdicts(I, k, case)
    finally:
        k.close()
