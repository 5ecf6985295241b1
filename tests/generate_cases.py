"""Shared by tests/test_generate_cpu.py and tests/test_gpu_generate.py: witnesses for
the action generators and the decomposition of a generated action into the pieces
the suite already pins (token_commit, prove_transfer / prove_issue, the writers of
fts_gpu.request)."""
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001  # BN254 group order


def bf(rng):
    return rng.randrange(R).to_bytes(32, "big")


def transfer_case(pp, rng, nin, nout, ttype=b"ABC", redeem_last=False, bits=None, extra=0):
    """(type, inputs, outputs): inputs [(tx_id, index, owner, com64, value, bf32)],
    outputs [(value, owner)] with sum(out) = sum(in) + extra"""
    bits = min(bits or pp.bit_length, 40)
    iv = [rng.randrange(1, 1 << (bits - 2)) for _ in range(nin)]
    tot = sum(iv) + extra
    ov = []
    for _ in range(nout - 1):
        ov.append(rng.randrange(tot - sum(ov) + 1))
    ov.append(tot - sum(ov))
    ins = []
    for k, v in enumerate(iv):
        b = bf(rng)
        ins.append((b"tx-%d" % rng.randrange(1 << 30), k, b"alice-%d" % k, pp.token_commit(ttype, v, b), v, b))
    outs = [(v, b"" if redeem_last and j == nout - 1 else b"bob-%d" % j) for j, v in enumerate(ov)]
    return ttype, ins, outs


def issue_case(pp, rng, nout, ttype=b"ABC", issuer=b"the-issuer"):
    """(type, issuer, outputs)"""
    return ttype, issuer, [(rng.randrange(1 << min(pp.bit_length, 40)), b"carol-%d" % j) for j in range(nout)]


def check_transfer_parts(pp, case, res, seed):
    """res = (action, metas, coms, bfs) of generate_transfer(case, seed) decomposes into
    token_commit, prove_transfer at the same seed and the request writers"""
    import fts_gpu as F
    ttype, ins, outs = case
    action, metas, coms, bfs = res
    assert len(metas) == len(coms) == len(bfs) == len(outs)
    for (v, _), c, b in zip(outs, coms, bfs):
        assert int.from_bytes(b, "big") < R
        assert c == pp.token_commit(ttype, v, b)
    proof = pp.prove_transfer(ttype, [i[4] for i in ins], [i[5] for i in ins], [o[0] for o in outs], bfs, seed)
    want = F.request.transfer_action([(tx, idx, owner, com) for tx, idx, owner, com, _, _ in ins],
                                     [(owner, c) for (_, owner), c in zip(outs, coms)], proof)
    assert action == want
    for (v, _), b, m in zip(outs, bfs, metas):
        assert m == F.request.token_metadata(ttype, v.to_bytes(32, "big"), b)
        assert F.decode_metadata(m) == (ttype, v.to_bytes(32, "big"), b)
    return proof


def check_issue_parts(pp, case, res, seed):
    import fts_gpu as F
    ttype, issuer, outs = case
    action, metas, coms, bfs = res
    assert len(metas) == len(coms) == len(bfs) == len(outs)
    for (v, _), c, b in zip(outs, coms, bfs):
        assert int.from_bytes(b, "big") < R
        assert c == pp.token_commit(ttype, v, b)
    proof = pp.prove_issue(ttype, [o[0] for o in outs], bfs, seed)
    assert action == F.request.issue_action(issuer, [(owner, c) for (_, owner), c in zip(outs, coms)], proof)
    for (v, _), b, m in zip(outs, bfs, metas):
        assert m == F.request.token_metadata(ttype, v.to_bytes(32, "big"), b, issuer=issuer)
        assert F.decode_metadata(m) == (ttype, v.to_bytes(32, "big"), b)
    return proof


def rng_for(name):
    return random.Random(name)
