"""CPU: whole transfer / issue actions on the host (fts_transfer_generate,
fts_issue_generate) -- Sender.GenerateZKTransfer (crypto/transfer/sender.go:54-107)
and Issuer.GenerateZKIssue (crypto/issue/issuer.go:39-84).

A generated action decomposes into pieces the suite already pins: every output
commitment is token_commit on the returned blinding factor, the proof is
prove_transfer / prove_issue at the same seed, the action and metadata bytes are
the writers of fts_gpu.request over those parts.  The C oracle accepts the
result, and rejects a transfer whose sums differ.  16-bit context: each case is
well under a second."""
import os
import subprocess

import pytest

from conftest import ROOT

import generate_cases as gc

BITS = 16
SHAPES = [(2, 2, False), (1, 1, False), (1, 2, False), (3, 1, True)]  # (n_in, n_out, last output redeems)


@pytest.fixture(scope="module")
def pp(host_pp):
    return host_pp(BITS)


@pytest.fixture(scope="module")
def opp(oracle_pp):
    return oracle_pp.with_bit_length(BITS)


@pytest.mark.parametrize("nin,nout,redeem", SHAPES)
def test_host_transfer_generation(pp, opp, nin, nout, redeem):
    import fts_gpu as F
    from oracle import cref
    case = gc.transfer_case(pp, gc.rng_for("cpu-t-%d-%d" % (nin, nout)), nin, nout, redeem_last=redeem)
    seed = 7000 + 10 * nin + nout
    res = pp.generate_transfer(*case, seed=seed)
    proof = gc.check_transfer_parts(pp, case, res, seed)
    if redeem:
        assert case[2][-1][1] == b""
    info = F.inspect_request(F.request.token_request([(F.request.TRANSFER, res[0])], [b"sig"]))
    assert (info["status"], info["n_issue"], info["n_transfer"]) == (F.FTS_OK, 0, 1)
    assert cref.action_verify_many(opp, [("transfer", [i[3] for i in case[1]], res[2], proof)]) == [(F.FTS_OK, -1)]


@pytest.mark.parametrize("nout", [1, 4])
def test_host_issue_generation(pp, opp, nout):
    import fts_gpu as F
    from oracle import cref
    case = gc.issue_case(pp, gc.rng_for("cpu-i-%d" % nout), nout)
    seed = 7100 + nout
    res = pp.generate_issue(*case, seed=seed)
    proof = gc.check_issue_parts(pp, case, res, seed)
    info = F.inspect_request(F.request.token_request([(F.request.ISSUE, res[0])], [b"sig"]))
    assert (info["status"], info["n_issue"], info["n_transfer"]) == (F.FTS_OK, 1, 0)
    assert cref.action_verify_many(opp, [("issue", [], res[2], proof)]) == [(F.FTS_OK, -1)]


def test_issue_without_issuer_and_type(pp):
    """proto3 empties: no type field in the metadata, an empty Identity in the action"""
    case = (b"", b"", [(5, b"o")])
    gc.check_issue_parts(pp, case, pp.generate_issue(*case, seed=7200), 7200)


def test_blinding_factors(pp, opp):
    """canonical, pairwise distinct, reproducible under a seed; fresh under FTS_SEED_OS_RANDOM"""
    import fts_gpu as F
    from oracle import cref
    case = gc.transfer_case(pp, gc.rng_for("cpu-bf"), 2, 4)
    a = pp.generate_transfer(*case, seed=7300)
    assert a == pp.generate_transfer(*case, seed=7300)
    assert a[3] != pp.generate_transfer(*case, seed=7301)[3]
    assert all(int.from_bytes(b, "big") < gc.R for b in a[3]) and len(set(a[3])) == 4
    s1 = pp.generate_transfer(*case, seed=F.FTS_SEED_OS_RANDOM)
    s2 = pp.generate_transfer(*case, seed=F.FTS_SEED_OS_RANDOM)
    assert not set(s1[3]) & set(s2[3]) and len(set(s1[3])) == 4 and len(set(s2[3])) == 4
    ins = [i[3] for i in case[1]]
    for s in (s1, s2):
        assert all(int.from_bytes(b, "big") < gc.R for b in s[3])
        for (v, _), c, b in zip(case[2], s[2], s[3]):
            assert c == pp.token_commit(case[0], v, b)
        # the proof is field 3 {1: bytes} of the action: the last bytes of it
        outs = [(o[1], c) for o, c in zip(case[2], s[2])]
        head = F.request.transfer_action([(i[0], i[1], i[2], i[3]) for i in case[1]], outs, None)
        assert s[0].startswith(head)
        proof = _proof_of(s[0][len(head):])
        assert cref.action_verify_many(opp, [("transfer", ins, s[2], proof)]) == [(F.FTS_OK, -1)]
    iss = gc.issue_case(pp, gc.rng_for("cpu-bf-i"), 2)
    i1 = pp.generate_issue(*iss, seed=F.FTS_SEED_OS_RANDOM)
    i2 = pp.generate_issue(*iss, seed=F.FTS_SEED_OS_RANDOM)
    assert not set(i1[3]) & set(i2[3])


def _varint(b, o):
    v = sh = 0
    while True:
        c = b[o]
        o += 1
        v |= (c & 0x7F) << sh
        sh += 7
        if not c & 0x80:
            return v, o


def _proof_of(tail):
    """Proof field (3: {1: proof}) that ends a TransferAction -> the proof bytes"""
    assert tail[0] == (3 << 3) | 2
    n, o = _varint(tail, 1)
    assert o + n == len(tail) and tail[o] == (1 << 3) | 2
    m, o = _varint(tail, o + 1)
    assert o + m == len(tail)
    return tail[o:]


def test_unbalanced_transfer_is_generated_and_rejected(pp, opp):
    """sum(in) != sum(out): no error from the generator (as in the reference); the C
    oracle rejects the proof, so the accepting cases above are not vacuous"""
    import fts_gpu as F
    from oracle import cref
    case = gc.transfer_case(pp, gc.rng_for("cpu-bad"), 2, 2, extra=1)
    res = pp.generate_transfer(*case, seed=7400)
    proof = gc.check_transfer_parts(pp, case, res, 7400)
    st = cref.action_verify_many(opp, [("transfer", [i[3] for i in case[1]], res[2], proof)])
    assert st == [(F.FTS_E_TAS_INVALID, -1)]


def test_device_entry_points_need_a_device(pp):
    import fts_gpu as F
    from fts_gpu import _lib as L
    t = gc.transfer_case(pp, gc.rng_for("cpu-nodev"), 1, 1)
    for call in (lambda: pp.generate_transfers_gpu([t], seed=1),
                 lambda: pp.generate_issues_gpu([gc.issue_case(pp, gc.rng_for("x"), 1)], seed=1),
                 lambda: pp.token_commit_batch_gpu([(b"ABC", 1, bytes(32))])):
        with pytest.raises(F.FtsError) as e:
            call()
        assert e.value.code == -3  # FTS_API_EDEVICE
    assert F.token_commit_batch_width() % 64 == 0 and F.token_commit_batch_width() >= 64
    assert hasattr(L.lib, "fts_transfer_generate_batch_gpu")


def test_generate_check():
    """lib/generate_check (csrc/tools/generate_check.cpp): the host generators and the
    serializers of host/action_write.hpp as a plain program built with the host address /
    undefined-behaviour sanitizers -- owners across the varint and DER length edges,
    exact-size and one-byte-short buffers"""
    exe = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "generate_check")
    gold = os.path.join(ROOT, "tests", "golden", "zkatdlog_pp.json")
    out = subprocess.run([exe, gold], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "generate_check: ok" in out.stdout
