"""GPU: the provers, the commit call and the generators on a multi-device context.

Every call splits over the children (fts_shard_plan with the verify side's weights),
item g of the caller's batch keeps randomness stream g on whichever child it runs, and
the parent packs once: seeded output is the single-device call's, byte for byte, and so
the host prover's at seed + g.  Equal bytes alone would also pass with one child doing
all the work, so every call is followed by a look at fts_debug_shard_work: each child's
counters moved by exactly its slice of the plan.

Contexts [0], [0, 0] and [0, 0, 0] at 16 bits put several shards on one GPU: the split,
thread and merge code that distinct devices run."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import generate_cases as gc

pytestmark = pytest.mark.gpu

EINVAL, EDEVICE, ESIZE = -1, -3, -5
CANARY = 0xA5
_MULTI = {}


def _multi(pp_raw, devices):
    import fts_gpu
    key = tuple(devices)
    if key not in _MULTI:
        _MULTI[key] = fts_gpu.PublicParams(pp_raw, bit_length=16, devices=list(devices))
    return _MULTI[key]


# ---------------------------------------------------------------- work accounting
# an item of a call: (range proofs, sigma proofs, tokens committed, weight in the split)
def _rp_item():
    return (1, 0, 0, 1.0)


def _tok_item():
    return (0, 0, 1, 1.0)


def _action_item(n_in, n_out, transfer, generated=False):
    rp = 0 if transfer and n_in == 1 and n_out == 1 else n_out  # transfer.go:85-87
    return (rp, 1, n_out if generated else 0, rp + 0.25)


class _Work:
    """shard_work of every child before a call; check(): each child's counters moved by its
    slice of fts_shard_plan, one pass per kind of work it had"""

    def __init__(self, pp):
        self.pp, self.ns = pp, len(pp.devices)
        self.before = self._read()

    def _read(self):
        return [self.pp.shard_work(j) for j in range(self.ns)]

    def delta(self):
        return [tuple(b - a for a, b in zip(x, y)) for x, y in zip(self.before, self._read())]

    def check(self, items, weighted):
        from fts_gpu import _lib as L
        b = L.shard_plan(len(items), self.ns, [it[3] for it in items] if weighted else None)
        want = []
        for j in range(self.ns):
            sl = items[b[j]:b[j + 1]]
            p, a, t = (sum(it[q] for it in sl) for q in range(3))
            want.append((p, a, t, (p > 0) + (a > 0) + (t > 0)))
        got = self.delta()
        for j in range(self.ns):
            if b[j + 1] > b[j]:
                assert got[j][3] >= 1, "child %d got items %d..%d and started no pass" % (j, b[j], b[j + 1])
        for q in range(3):
            assert sum(g[q] for g in got) == sum(it[q] for it in items)
        assert got == want
        return b


# ---------------------------------------------------------------- raw calls
def _rp_raw(pp, vals, bfs, seed, cap=None):
    """fts_rp_prove_batch_gpu -> (rc, out, offsets, lens, com64)"""
    from fts_gpu import _lib as L
    n = len(vals)
    cap = n * (1500 + 150 * pp.rounds) + 4096 if cap is None else cap
    out = np.full(max(1, cap), CANARY, dtype=np.uint8)
    offs, lens = (C.c_size_t * n)(), (C.c_size_t * n)()
    coms = np.zeros(64 * n, dtype=np.uint8)
    rc = L.lib.fts_rp_prove_batch_gpu(pp._ctx, n, (C.c_uint64 * n)(*vals), b"".join(bfs), seed, out.ctypes.data, cap,
                                      offs, lens, coms.ctypes.data)
    return rc, out.tobytes(), list(offs), list(lens), coms.tobytes()


def _act_raw(pp, fn, wb, seed, cap=None):
    """fts_transfer_prove_batch_gpu / fts_issue_prove_batch_gpu -> (rc, out, offsets, lens)"""
    from fts_gpu import _lib as L
    cap = wb.cap if cap is None else cap
    out = np.full(max(1, cap), CANARY, dtype=np.uint8)
    offs, lens = (C.c_size_t * wb.n)(), (C.c_size_t * wb.n)()
    rc = getattr(L.lib, fn)(pp._ctx, wb.n, wb.items, seed, out.ctypes.data, cap, offs, lens)
    return rc, out.tobytes(), list(offs), list(lens)


def _gen_raw(pp, fn, gb, seed, acap=None, mcap=None):
    """fts_*_generate_batch_gpu into canary-filled buffers -> (rc, everything the call writes)"""
    from fts_gpu import _lib as L
    r = gb.result()
    for a in (r.actions, r.meta, r.com, r.bf):
        a[:] = CANARY
    if acap is not None:
        r.c.actions_cap = acap
    if mcap is not None:
        r.c.meta_cap = mcap
    rc = getattr(L.lib, fn)(pp._ctx, gb.n, gb.items, seed, C.byref(r.c))
    return rc, {"actions": r.actions.tobytes(), "meta": r.meta.tobytes(), "aoff": list(r.aoff), "alen": list(r.alen),
                "moff": list(r.moff), "mlen": list(r.mlen), "com64": r.com.tobytes(), "bf32": r.bf.tobytes()}


def _proofs(out, offs, lens):
    return [out[o:o + ln] for o, ln in zip(offs, lens)]


# ---------------------------------------------------------------- cases
def _rp_case(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1 << 16) for _ in range(n)], [gc.bf(rng) for _ in range(n)]


def _transfer_witnesses(n, seed):
    """1-in/1-out (no range proof: weight 0.25), 2-in/2-out and 3-in/1-out, mixed"""
    rng = random.Random(seed)
    shapes = [(1, 1), (2, 2), (3, 1), (2, 2), (1, 1)]
    out = []
    for i in range(n):
        nin, nout = shapes[i % len(shapes)]
        iv = [rng.randrange(1, 1 << 13) for _ in range(nin)]
        ov = [rng.randrange(sum(iv) + 1)] if nout == 2 else []
        ov.append(sum(iv) - sum(ov))
        out.append((b"ABC" if i % 3 else b"USD", iv, [gc.bf(rng) for _ in iv], ov, [gc.bf(rng) for _ in ov]))
    return out


def _issue_witnesses(n, seed):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        m = 1 + i % 4
        out.append((b"EUR", [], [], [rng.randrange(1 << 16) for _ in range(m)], [gc.bf(rng) for _ in range(m)]))
    return out


def _gen_transfers(pp, n, tag):
    rng = gc.rng_for(tag)
    shapes = [(2, 2), (1, 1), (1, 2), (3, 1), (2, 3)]
    return [gc.transfer_case(pp, rng, *shapes[i % 5], ttype=b"ABC" if i % 2 else b"USD", redeem_last=(i % 5 == 3))
            for i in range(n)]


def _gen_issues(pp, n, tag):
    rng = gc.rng_for(tag)
    return [gc.issue_case(pp, rng, 1 + i % 4) for i in range(n)]


def _gen_batches(F, pp, transfers, issues):
    return (F.GenBatch([(t, i, o, b"") for t, i, o in transfers], pp.rounds),
            F.GenBatch([(t, [], o, iss) for t, iss, o in issues], pp.rounds))


# ---------------------------------------------------------------- 1. range proofs
@pytest.fixture(scope="module")
def rp_reference(gpu_pp, host_pp):
    """37 proofs on the single-device context, equal to the host prover's (computed once)"""
    vals, bfs = _rp_case(37, 1)
    rc, out, offs, lens, coms = _rp_raw(gpu_pp(16), vals, bfs, 41000)
    assert rc == 0
    hp, hc = host_pp(16).prove_range_batch(vals, bfs, 41000)
    assert _proofs(out, offs, lens) == hp and coms == b"".join(hc)
    return vals, bfs, (out[:offs[-1] + lens[-1]], offs, lens, coms)


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_range_proofs_split_over_every_child(pp_raw, rp_reference, devices):
    vals, bfs, (out1, offs1, lens1, coms1) = rp_reference
    multi = _multi(pp_raw, devices)
    w = _Work(multi)
    rc, out, offs, lens, coms = _rp_raw(multi, vals, bfs, 41000)
    assert rc == 0
    w.check([_rp_item()] * 37, False)
    assert (offs, lens, coms) == (offs1, lens1, coms1)
    assert out[:len(out1)] == out1


@pytest.mark.parametrize("n", [1, 2])
def test_range_proofs_fewer_than_children(pp_raw, gpu_pp, host_pp, n):
    """empty shards are skipped"""
    multi = _multi(pp_raw, [0, 0, 0])
    vals, bfs = _rp_case(n, 2)
    w = _Work(multi)
    got = multi.prove_range_batch_gpu(vals, bfs, 41100)
    b = w.check([_rp_item()] * n, False)
    assert sum(1 for j in range(3) if b[j + 1] > b[j]) == n
    assert got == gpu_pp(16).prove_range_batch_gpu(vals, bfs, 41100) == host_pp(16).prove_range_batch(vals, bfs, 41100)


# ---------------------------------------------------------------- 2. action proofs
@pytest.mark.parametrize("kind,n", [("transfer", 23), ("issue", 11)])
def test_action_proofs_equal_single_device(pp_raw, gpu_pp, host_pp, kind, n):
    import fts_gpu as F
    single, host = gpu_pp(16), host_pp(16)
    transfer = kind == "transfer"
    wit = _transfer_witnesses(n, 3) if transfer else _issue_witnesses(n, 4)
    fn = "fts_%s_prove_batch_gpu" % kind
    wb = F.WitnessBatch(wit, single.rounds)
    rc, out1, offs1, lens1 = _act_raw(single, fn, wb, 42000)
    assert rc == 0
    want = _proofs(out1, offs1, lens1)
    for g in (0, 1, n // 2, n - 1):
        t, iv, ib, ov, ob = wit[g]
        assert want[g] == (host.prove_transfer(t, iv, ib, ov, ob, 42000 + g) if transfer
                           else host.prove_issue(t, ov, ob, 42000 + g)), g
    items = [_action_item(len(x[1]), len(x[3]), transfer) for x in wit]
    for devices in ([0, 0], [0, 0, 0]):
        multi = _multi(pp_raw, devices)
        w = _Work(multi)
        rc, out, offs, lens = _act_raw(multi, fn, wb, 42000)
        assert rc == 0
        w.check(items, True)
        assert (offs, lens) == (offs1, lens1) and out == out1


# ---------------------------------------------------------------- 3. generation
@pytest.mark.parametrize("kind,n", [("transfer", 13), ("issue", 9)])
def test_generation_equals_single_device_and_host(pp_raw, gpu_pp, kind, n):
    import fts_gpu as F
    single = gpu_pp(16)
    transfer = kind == "transfer"
    cases = _gen_transfers(single, n, "pm-gt") if transfer else _gen_issues(single, n, "pm-gi")
    gt, gi = _gen_batches(F, single, cases if transfer else [], [] if transfer else cases)
    gb = gt if transfer else gi
    fn = "fts_%s_generate_batch_gpu" % kind
    rc, ref = _gen_raw(single, fn, gb, 43000)
    assert rc == 0
    n_out = [len(c[2]) for c in cases]
    items = [_action_item(len(c[1]) if transfer else 0, m, transfer, generated=True) for c, m in zip(cases, n_out)]
    host_gen = single.generate_transfer if transfer else single.generate_issue
    for devices in ([0, 0], [0, 0, 0]):
        multi = _multi(pp_raw, devices)
        w = _Work(multi)
        rc, got = _gen_raw(multi, fn, gb, 43000)
        assert rc == 0
        b = w.check(items, True)
        assert got == ref
        # outputs are numbered across the shards: the first action of the second shard
        # has its commitments and blinding factors at the call's offsets, and every
        # sampled action is the host's at seed + i
        assert 0 < b[1] < n
        for i in sorted({0, b[1], b[-2], n - 1}):
            t0 = sum(n_out[:i])
            action, metas, coms, bfs = host_gen(*cases[i], seed=43000 + i)
            assert got["actions"][got["aoff"][i]:got["aoff"][i] + got["alen"][i]] == action, i
            for j in range(n_out[i]):
                t = t0 + j
                assert got["com64"][64 * t:64 * t + 64] == coms[j] and got["bf32"][32 * t:32 * t + 32] == bfs[j]
                assert got["meta"][got["moff"][t]:got["moff"][t] + got["mlen"][t]] == metas[j]


# ---------------------------------------------------------------- 4. commit
@pytest.mark.parametrize("n", [0, 1, 65])
def test_commit_on_three_shards(pp_raw, gpu_pp, host_pp, n):
    multi = _multi(pp_raw, [0, 0, 0])
    rng = random.Random(n)
    items = [((b"ABC", b"", b"a-longer-token-type")[i % 3], rng.randrange(1 << 64), gc.bf(rng)) for i in range(n)]
    w = _Work(multi)
    got = multi.token_commit_batch_gpu(items)
    w.check([_tok_item()] * n, False)
    assert got == gpu_pp(16).token_commit_batch_gpu(items)
    assert got == [host_pp(16).token_commit(*it) for it in items]


# ---------------------------------------------------------------- 5. ESIZE
def test_generation_esize_leaves_the_buffers_untouched(pp_raw, gpu_pp):
    import fts_gpu as F
    single, multi = gpu_pp(16), _multi(pp_raw, [0, 0])
    cases = _gen_transfers(single, 7, "pm-es")
    gb, _ = _gen_batches(F, single, cases, [])
    items = [_action_item(len(c[1]), len(c[2]), True, generated=True) for c in cases]
    fn = "fts_transfer_generate_batch_gpu"
    rc, full = _gen_raw(single, fn, gb, 44000)
    assert rc == 0
    need_a, need_m = full["aoff"][-1] + full["alen"][-1], full["moff"][-1] + full["mlen"][-1]
    for caps in ({"acap": need_a - 1}, {"mcap": need_m - 1}):
        rc1, ref = _gen_raw(single, fn, gb, 44000, **caps)
        w = _Work(multi)
        rc2, got = _gen_raw(multi, fn, gb, 44000, **caps)
        w.check(items, True)
        assert rc1 == rc2 == ESIZE
        for k in ("aoff", "alen", "moff", "mlen"):
            assert got[k] == ref[k] == full[k], k
        assert set(got["actions"]) == set(got["meta"]) == {CANARY}
    # and with exactly enough room it fits
    rc, got = _gen_raw(multi, fn, gb, 44000, acap=need_a, mcap=need_m)
    assert rc == 0 and got["actions"][:need_a] == full["actions"][:need_a]


def test_prover_esize_fills_the_same_prefix(pp_raw, gpu_pp):
    import fts_gpu as F
    single, multi = gpu_pp(16), _multi(pp_raw, [0, 0])
    vals, bfs = _rp_case(9, 5)
    rc, _, offs, lens, _ = _rp_raw(single, vals, bfs, 44100)
    assert rc == 0
    cap = offs[5] + lens[5] - 1  # proof 5 is the first that does not fit
    rc1, _, offs1, lens1, coms1 = _rp_raw(single, vals, bfs, 44100, cap=cap)
    w = _Work(multi)
    rc2, _, offs2, lens2, coms2 = _rp_raw(multi, vals, bfs, 44100, cap=cap)
    w.check([_rp_item()] * 9, False)
    assert rc1 == rc2 == ESIZE
    assert (offs2, lens2, coms2) == (offs1, lens1, coms1) and offs2[:6] == offs[:6] and lens2[:6] == lens[:6]
    wit = _transfer_witnesses(9, 6)
    wb = F.WitnessBatch(wit, single.rounds)
    fn = "fts_transfer_prove_batch_gpu"
    rc, _, offs, lens = _act_raw(single, fn, wb, 44200)
    assert rc == 0
    cap = offs[6] + lens[6] - 1
    rc1, _, offs1, lens1 = _act_raw(single, fn, wb, 44200, cap=cap)
    w = _Work(multi)
    rc2, _, offs2, lens2 = _act_raw(multi, fn, wb, 44200, cap=cap)
    w.check([_action_item(len(x[1]), len(x[3]), True) for x in wit], True)
    assert rc1 == rc2 == ESIZE
    assert (offs2, lens2) == (offs1, lens1) and offs2[:7] == offs[:7] and lens2[:7] == lens[:7]


# ---------------------------------------------------------------- 6. EINVAL before work
def test_invalid_item_in_the_last_shard_starts_no_work(pp_raw, gpu_pp):
    import fts_gpu as F
    single, multi = gpu_pp(16), _multi(pp_raw, [0, 0, 0])
    wit = _transfer_witnesses(12, 7)
    t, iv, ib, _, _ = wit[-1]
    wit[-1] = (t, iv, ib, [], [])  # n_out = 0
    w = _Work(multi)
    rc, _, _, _ = _act_raw(multi, "fts_transfer_prove_batch_gpu", F.WitnessBatch(wit, single.rounds), 45000)
    assert rc == EINVAL
    assert w.delta() == [(0, 0, 0, 0)] * 3
    cases = _gen_transfers(single, 12, "pm-ei")
    t, ins, _ = cases[-1]
    cases[-1] = (t, ins, [])
    gb, _ = _gen_batches(F, single, cases, [])
    rc, _ = _gen_raw(multi, "fts_transfer_generate_batch_gpu", gb, 45100)
    assert rc == EINVAL
    assert w.delta() == [(0, 0, 0, 0)] * 3
    from fts_gpu import _lib as L
    items = (L.CommitItem * 9)()
    keep = [C.create_string_buffer(bytes(32), 32) for _ in range(8)]
    for i, b in enumerate(keep):
        items[i] = L.CommitItem(None, 0, i, C.cast(b, C.c_void_p))  # item 8: bf32 NULL
    out = C.create_string_buffer(64 * 9)
    assert L.lib.fts_token_commit_batch_gpu(multi._ctx, 9, items, out) == EINVAL
    assert w.delta() == [(0, 0, 0, 0)] * 3


# ---------------------------------------------------------------- 7. secure mode
def _last_field(action, prefix):
    """the proof of a generated action: its last field, {1: proof}, after the fields
    the request writers give for the same inputs and outputs"""
    assert action.startswith(prefix)

    def ld(b, p):  # (tag, payload, next) of a length-delimited field
        tag, n, sh = b[p], 0, 0
        p += 1
        while True:
            n |= (b[p] & 0x7F) << sh
            sh += 7
            p += 1
            if not b[p - 1] & 0x80:
                return tag, b[p:p + n], p + n
    _, body, end = ld(action, len(prefix))
    assert end == len(action)
    tag, proof, end = ld(body, 0)
    assert tag == 0x0A and end == len(body)
    return proof


def _range_proof_Cs(proof):
    from oracle import der, zkat
    _, rc = der.unmarshal_values(proof)
    return [repr(zkat.RangeProof.deserialize(rp).data.C) for rp in der.unmarshal_values(der.unmarshal_values(rc)[0])]


def test_secure_mode_shares_no_stream(pp_raw, gpu_pp):
    import fts_gpu as F
    single, multi = gpu_pp(16), _multi(pp_raw, [0, 0, 0])
    rng = gc.rng_for("pm-sec")
    trs = [gc.transfer_case(single, rng, 2, 2) for _ in range(9)]
    iss = [gc.issue_case(single, rng, 2) for _ in range(5)]
    w = _Work(multi)
    gt = multi.generate_transfers_gpu(trs, seed=F.FTS_SEED_OS_RANDOM)
    w.check([_action_item(2, 2, True, generated=True)] * 9, True)
    w = _Work(multi)
    gi = multi.generate_issues_gpu(iss, seed=F.FTS_SEED_OS_RANDOM)
    w.check([_action_item(0, 2, False, generated=True)] * 5, True)
    titems, iitems = [], []
    for (t, ins, outs), (action, _, coms, _) in zip(trs, gt):
        prefix = F.request.transfer_action([(tx, idx, owner, com) for tx, idx, owner, com, _, _ in ins],
                                           [(owner, c) for (_, owner), c in zip(outs, coms)], None)
        titems.append(([i[3] for i in ins], coms, _last_field(action, prefix)))
    for (t, issuer, outs), (action, _, coms, _) in zip(iss, gi):
        prefix = F.request.issue_action(issuer, [(owner, c) for (_, owner), c in zip(outs, coms)], None)
        iitems.append((coms, _last_field(action, prefix)))
    before = single.pass_stats()
    st, _ = single.verify_transfers(titems)
    assert [int(s) for s in st] == [F.FTS_OK] * 9
    st, _ = single.verify_issues(iitems)
    assert [int(s) for s in st] == [F.FTS_OK] * 5
    d = tuple(b - a for a, b in zip(before, single.pass_stats()))
    assert d[0] >= 1 and d[1:] == (0, 0, 0)
    bfs = [b for g in gt + gi for b in g[3]]
    assert len(bfs) == 28 and len(set(bfs)) == 28
    Cs = [c for it in titems for c in _range_proof_Cs(it[2])] + [c for it in iitems for c in _range_proof_Cs(it[1])]
    assert len(Cs) == 28 and len(set(Cs)) == 28


# ---------------------------------------------------------------- 8. concurrency
def test_two_concurrent_generate_calls(pp_raw, gpu_pp):
    import fts_gpu as F
    single, multi = gpu_pp(16), _multi(pp_raw, [0, 0])
    cases = _gen_transfers(single, 10, "pm-cc")
    batches = [_gen_batches(F, single, cases, [])[0] for _ in range(2)]
    seeds = [46000, 47000]
    serial = [multi.generate_transfers_gpu(batches[k], seed=seeds[k]) for k in range(2)]
    assert serial[0] != serial[1]
    got = [None, None]

    def run(k):
        got[k] = multi.generate_transfers_gpu(batches[k], seed=seeds[k])
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == serial
