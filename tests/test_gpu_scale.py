"""GPU: BASELINE config C2 at full size (4,096 standalone 64-bit range proofs
in one batch) through size-independent properties: every honest proof is
accepted, exactly the tampered positions are rejected with the reference's
error class, and re-verifying the staged batch is idempotent."""
import random

import pytest

from oracle import bn254 as bn, zkat

pytestmark = pytest.mark.gpu


def test_full_batch_4096_rp64(gpu_pp):
    pp = gpu_pp(64)
    n = 4096
    rng = random.Random(0xF7A50002)
    vals = [rng.getrandbits(64) for _ in range(n)]
    bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(n)]
    proofs, coms = pp.prove_range_batch(vals, bfs, seed=0xF7A50002)
    b = pp.stage_range_proofs(proofs, coms)
    st = b.verify()
    assert int((st != 0).sum()) == 0
    # 1% tampered: random T1 (-> invalid range proof) or L_j (-> invalid IPA)
    bad = sorted(rng.sample(range(n), 41))
    kinds = {}
    for i in bad:
        r = zkat.RangeProof.deserialize(proofs[i])
        if rng.random() < 0.5:
            r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
            kinds[i] = 3
        else:
            j = rng.randrange(6)
            r.ipa.L[j] = bn.g1_add(r.ipa.L[j], bn.GEN)
            kinds[i] = 6
        proofs[i] = r.serialize()
    b2 = pp.stage_range_proofs(proofs, coms)
    st2 = b2.verify()
    assert {i: int(st2[i]) for i in range(n) if st2[i] != 0} == kinds
    assert (b2.verify() == st2).all()
    b.close()
    b2.close()


def test_concurrent_lanes_rp32(gpu_pp):
    """Concurrent fts_rp_batch_verify calls on different staged batches run on
    different device lanes (stream pairs + workspaces): every batch must still
    get exactly its own verdicts (tampered positions differ per batch)."""
    import threading

    pp = gpu_pp(32)
    rng = random.Random(0xF7A5C0DE)
    batches, expect = [], []
    for t in range(4):
        m = 96
        vals = [rng.getrandbits(32) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch(vals, bfs, seed=1000 + t)
        bad = set(rng.sample(range(m), 3 + t))
        for i in bad:
            r = zkat.RangeProof.deserialize(proofs[i])
            r.data.T2 = bn.g1_add(r.data.T2, bn.GEN)
            proofs[i] = r.serialize()
        batches.append(pp.stage_range_proofs(proofs, coms))
        expect.append([3 if i in bad else 0 for i in range(m)])
    out = [[] for _ in batches]

    def work(t):
        for _ in range(3):
            out[t].append([int(s) for s in batches[t].verify()])

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(batches))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(len(batches)):
        assert len(out[t]) == 3
        for st in out[t]:
            assert st == expect[t]
        batches[t].close()


def _one_lane_ctx(pp_raw):
    """a 16-bit context with ONE device lane, whose idle window is off
    (FTS_IDLE_GATHER_US=0); tests queue their submissions with pp.hold(n)
    (fts_debug_hold) so they coalesce deterministically"""
    import os

    import fts_gpu
    saved = {k: os.environ.get(k) for k in ("FTS_LANES", "FTS_IDLE_GATHER_US")}
    os.environ.update(FTS_LANES="1", FTS_IDLE_GATHER_US="0")
    try:
        return fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_coalesced_batches_keep_their_verdicts(pp_raw):
    """With ONE device lane, batches submitted concurrently are coalesced into
    shared device passes (fts_rp_batch_verify's dispatcher).  Each caller must
    still get exactly its own per-proof verdicts, including the per-proof
    fallback (tampered proofs make the merged combination fail)."""
    import os
    import threading

    import fts_gpu

    pp = _one_lane_ctx(pp_raw)
    rng = random.Random(0xC0A1E5CE)
    sizes = [1, 7, 64, 200, 33, 128, 5, 90]
    batches, expect = [], []
    for t, m in enumerate(sizes):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch(vals, bfs, seed=5000 + t)
        exp = [0] * m
        if t % 2 == 1:  # odd batches carry tampered proofs of both classes
            for i in rng.sample(range(m), min(m, 2 + t // 2)):
                r = zkat.RangeProof.deserialize(proofs[i])
                if rng.random() < 0.5:
                    r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
                    exp[i] = 3
                else:
                    r.ipa.R[rng.randrange(4)] = bn.g1_add(r.ipa.R[0], bn.GEN)
                    exp[i] = 6
                proofs[i] = r.serialize()
        batches.append(pp.stage_range_proofs(proofs, coms))
        expect.append(exp)
    out = [[] for _ in batches]
    merged = []

    def work(t):
        for _ in range(4):
            out[t].append([int(s) for s in batches[t].verify()])
            merged.append(batches[t].merged())

    pp.hold(len(batches))  # fts_debug_hold: the first submissions form one pass
    th = [threading.Thread(target=work, args=(t,)) for t in range(len(batches))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(len(batches)):
        assert len(out[t]) == 4
        for st in out[t]:
            assert st == expect[t], t
    assert max(merged) > 1, merged  # the dispatcher did merge batches
    for b in batches:
        b.close()
    pp.close()


@pytest.mark.parametrize("main_groups", [0, 1])
def test_one_bad_proof_in_coalesced_pass_group_test(pp_raw, main_groups):
    """SURVEY Appendix B fallback: one tampered proof inside a coalesced pass of 8
    caller batches.  The failed batch check is narrowed by group tests (groups never
    straddle two caller batches) so only a handful of proofs -- all of the bad
    proof's own batch -- get the per-proof final equations; every verdict equals
    the reference's (rangecorrectness.go:141-160).  FTS_MAIN_GROUPS=1: the pass
    checks one combination per caller batch, so the group test covers the bad
    proof's batch only; 0 (default): one combination over the pass, whose single
    bad proof the locator finds (round 5; the group test only when it misses)."""
    import os
    import threading

    import fts_gpu

    saved = {k: os.environ.get(k) for k in ("FTS_LANES", "FTS_MAIN_GROUPS", "FTS_IDLE_GATHER_US")}
    os.environ.update(FTS_LANES="1", FTS_MAIN_GROUPS=str(main_groups))
    os.environ["FTS_IDLE_GATHER_US"] = "0"  # no idle window: the held queue forms its pass at once
    try:
        pp = fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    rng = random.Random(0xB15EC7)
    m, nb, bad_batch, bad_idx = 512, 8, 3, 333
    batches, expect = [], []
    for t in range(nb):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=7000 + 1000 * t)
        exp = [0] * m
        if t == bad_batch:
            r = zkat.RangeProof.deserialize(proofs[bad_idx])
            r.ipa.L[1] = bn.g1_add(r.ipa.L[1], bn.GEN)
            proofs[bad_idx] = r.serialize()
            exp[bad_idx] = 6
        batches.append(pp.stage_range_proofs(proofs, coms))
        expect.append(exp)
    out, merged, tim = [None] * nb, [0] * nb, [None] * nb

    def work(t):
        out[t] = [int(s) for s in batches[t].verify()]
        merged[t] = batches[t].merged()
        tim[t] = batches[t].timings()

    pp.hold(nb)  # fts_debug_hold: the 8 submissions queue up and form one pass
    th = [threading.Thread(target=work, args=(t,)) for t in range(nb)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(nb):
        assert out[t] == expect[t], t
    assert merged == [nb] * nb, merged
    tb = tim[bad_batch]
    per_proof = tb["fb:k_rp_terms_fixed"][1] / ((3 + 2 * 16) * 15 * 11 * 136)
    if not main_groups:
        # one combination over the pass: the single-fault locator (rp_locate_single)
        # finds the bad proof; only its own per-proof equations run, no group test
        assert "fb:k_rlc_locate" in tb and "fb:k_rlc_group_final" not in tb, sorted(tb)
        assert round(per_proof) == 1, per_proof
    else:
        assert "fb:k_rlc_group_final" in tb and "fb:k_rp_terms_fixed" in tb, sorted(tb)
        # the bad proof's round-1 group (256 proofs of its own batch), not the pass (4,096)
        assert 1 <= round(per_proof) <= 256, per_proof
        # the group test's grouped sums: the bad proof's own batch (512 proofs) only
        grouped = tb["fb:k_rlc_group_columns"][1] / (4 * 16 * 136)
        assert round(grouped) == m, (grouped, merged[bad_batch])
    for b in batches:
        b.close()
    pp.close()


def _raw_timing_names(batch):
    """every timeline entry name of a staged batch's last verify (duplicates kept)"""
    import ctypes as C

    from fts_gpu import _lib as L
    names = (C.c_char_p * 128)()
    ms = (C.c_float * 128)()
    mads = (C.c_double * 128)()
    m = L.lib.fts_rp_batch_timings(batch._b, names, ms, mads, 128)
    return [names[i].decode() for i in range(m)], {names[i].decode(): mads[i] for i in range(m)}


def test_group_test_round2_exact_verdicts(pp_raw):
    """the group test's second round (api_rp.cpp
    rp_group_fallback: failing round-1 groups re-grouped by 8 over the compacted
    survivors) decides which proofs are accepted without their per-proof
    equations.  Forced here (FTS_GT1=64, FTS_GT2_MIN=0) on a coalesced pass of 3
    caller batches with tampered proofs in every batch: two in one round-2 group,
    two straddling a round-1 group boundary, the pass's last proof; two tamper
    kinds (T1 -> E1 fails, L_j -> E2 fails).  Every verdict must equal the
    oracle's, the group test must run twice, and only round-2 groups may reach
    the per-proof stage."""
    import os
    import threading

    import fts_gpu

    saved = {k: os.environ.get(k) for k in ("FTS_LANES", "FTS_GT1", "FTS_GT2_MIN", "FTS_IDLE_GATHER_US")}
    os.environ.update(FTS_LANES="1", FTS_GT1="64", FTS_GT2_MIN="0")
    os.environ["FTS_IDLE_GATHER_US"] = "0"  # no idle window: the held queue forms its pass at once
    try:
        pp = fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    from oracle import pp as oppm
    opp = oppm.load_pp(pp_raw).with_bit_length(16)
    rng = random.Random(0x6E0C2)
    m, nb = 384, 3
    bad = {0: {5: "T1", 6: "L"}, 1: {63: "L", 64: "T1", 200: "L"}, 2: {383: "T1"}}
    batches, expect = [], []
    for t in range(nb):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=8100 + 1000 * t)
        exp = [0] * m
        for i, kind in bad.get(t, {}).items():
            r = zkat.RangeProof.deserialize(proofs[i])
            if kind == "T1":
                r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
            else:
                j = rng.randrange(4)
                r.ipa.L[j] = bn.g1_add(r.ipa.L[j], bn.GEN)
            proofs[i] = r.serialize()
            err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q,
                                 opp.rounds, 16, zkat.RangeProof.deserialize(proofs[i]))
            assert err is not None
            exp[i] = fts_gpu.FTS_E_RP_INVALID if "IPA" not in err else fts_gpu.FTS_E_IPA_INVALID
        batches.append(pp.stage_range_proofs(proofs, coms))
        expect.append(exp)
    out, merged, names, work = [None] * nb, [0] * nb, [None] * nb, [None] * nb

    def run(t):
        out[t] = [int(s) for s in batches[t].verify()]
        merged[t] = batches[t].merged()
        names[t], work[t] = _raw_timing_names(batches[t])

    pp.hold(nb)  # fts_debug_hold: every caller batch in one pass
    th = [threading.Thread(target=run, args=(t,)) for t in range(nb)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(nb):
        assert out[t] == expect[t], (t, {i: (out[t][i], expect[t][i]) for i in range(m) if out[t][i] != expect[t][i]})
    # find a batch whose pass held every caller batch (the usual case); the last
    # one to finish carries that pass's timeline
    assert merged == [nb] * nb, merged
    full = list(range(nb))
    nm = names[full[0]]
    assert nm.count("fb:k_rlc_group_final") == 2, nm       # round 1 and round 2 ran
    per_proof = work[full[0]]["fb:k_rp_terms_fixed"] / ((3 + 2 * 16) * 15 * 11 * 136)
    nbad = sum(len(v) for v in bad.values())
    assert 1 <= round(per_proof) <= 8 * nbad, per_proof     # round-2 groups, not round-1 groups of 64
    for b in batches:
        b.close()
    pp.close()


def test_group_test_adaptive_dense_exact_verdicts(pp_raw):
    """api_rp.cpp rp_group_fallback, FTS_GT_ADAPT (default on): after a failed
    verification whose bad proofs were dense (more than half the batch's proofs
    in failing 256-groups) THAT caller batch starts its next fallback at groups
    of 8 on the small-group kernels, with no second round.  One caller batch of
    512 rp16 proofs, 16 of them tampered (every 32nd: both 256-groups fail),
    verified twice on one lane: both calls must give the oracle's verdicts; the
    first runs the 256-group kernels, the second only the small-group ones and
    sends at most the 16 failing 8-groups to the per-proof stage.  The state is
    per caller batch: another staged batch with two bad proofs (a miss
    of the single-fault locator), verified after it on the same context, still starts
    at groups of 256."""
    import os

    import fts_gpu

    saved = {k: os.environ.get(k) for k in ("FTS_LANES", "FTS_GT1", "FTS_GT2_MIN", "FTS_GT_ADAPT", "FTS_IDLE_GATHER_US")}
    for k in ("FTS_GT1", "FTS_GT2_MIN", "FTS_GT_ADAPT"):
        os.environ.pop(k, None)
    os.environ["FTS_LANES"] = "1"
    os.environ["FTS_IDLE_GATHER_US"] = "0"  # no idle window: the held queue forms its pass at once
    try:
        pp = fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    from oracle import pp as oppm
    opp = oppm.load_pp(pp_raw).with_bit_length(16)
    rng = random.Random(0xAD4F7)
    m = 512
    vals = [rng.getrandbits(16) for _ in range(m)]
    bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
    proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=9300)
    expect = [0] * m
    for i in range(7, m, 32):
        r = zkat.RangeProof.deserialize(proofs[i])
        if (i // 32) % 2:
            r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
        else:
            j = rng.randrange(4)
            r.ipa.L[j] = bn.g1_add(r.ipa.L[j], bn.GEN)
        proofs[i] = r.serialize()
        err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q,
                             opp.rounds, 16, zkat.RangeProof.deserialize(proofs[i]))
        assert err is not None
        expect[i] = fts_gpu.FTS_E_RP_INVALID if "IPA" not in err else fts_gpu.FTS_E_IPA_INVALID
    batch = pp.stage_range_proofs(proofs, coms)
    runs = []
    for _ in range(2):
        out = [int(s) for s in batch.verify()]
        assert out == expect, {i: (out[i], expect[i]) for i in range(m) if out[i] != expect[i]}
        runs.append(_raw_timing_names(batch))
    (n1, _), (n2, w2) = runs
    assert "fb:k_rlc_group_columns" in n1 and n1.count("fb:k_rlc_group_final") == 1, n1
    assert "fb:k_rlc_group_columns" not in n2 and "fb:k_rlc_group_cols" in n2, n2
    assert n2.count("fb:k_rlc_group_final") == 1, n2   # groups of 8, no second round
    per_proof = w2["fb:k_rp_terms_fixed"] / ((3 + 2 * 16) * 15 * 11 * 136)
    assert 1 <= round(per_proof) <= 8 * 16, per_proof
    # a second caller's batch: one bad proof, its own (sparse) group size
    vals2 = [rng.getrandbits(16) for _ in range(m)]
    bfs2 = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
    proofs2, coms2 = pp.prove_range_batch_gpu(vals2, bfs2, seed=9400)
    for i in (300, 310):  # two bad proofs in one 256-group: the single-fault locator misses
        r = zkat.RangeProof.deserialize(proofs2[i])
        r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
        proofs2[i] = r.serialize()
    other = pp.stage_range_proofs(proofs2, coms2)
    out2 = [int(s) for s in other.verify()]
    assert out2 == [fts_gpu.FTS_E_RP_INVALID if i in (300, 310) else 0 for i in range(m)]
    n3, _ = _raw_timing_names(other)
    assert "fb:k_rlc_group_columns" in n3 and "fb:k_rlc_group_cols" not in n3, n3
    # and the dense batch keeps its own state
    out = [int(s) for s in batch.verify()]
    assert out == expect
    n4, _ = _raw_timing_names(batch)
    assert "fb:k_rlc_group_cols" in n4 and "fb:k_rlc_group_columns" not in n4, n4
    other.close()
    batch.close()
    pp.close()


def test_dense_and_sparse_batches_in_one_pass(pp_raw):
    """one coalesced pass holding a DENSE caller batch (its last
    failure had many bad proofs: its group test starts at groups of 8) and a SPARSE
    one (one bad proof: groups of 256).  Both group tests upload their MSM window
    tables back to back with no sync between them (rp_group_fallback), from
    separate pinned slots; every verdict must be the oracle's, and the per-proof
    stage must see only the failing small groups and the sparse batch's one 256-group
    -- not every proof of the pass."""
    import os
    import threading

    import fts_gpu

    pp = _one_lane_ctx(pp_raw)
    from oracle import pp as oppm
    opp = oppm.load_pp(pp_raw).with_bit_length(16)
    rng = random.Random(0xD5A5)
    m = 512

    def make(seed, bad):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=seed)
        exp = [0] * m
        for i in bad:
            r = zkat.RangeProof.deserialize(proofs[i])
            if i % 2:
                r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
            else:
                j = rng.randrange(4)
                r.ipa.L[j] = bn.g1_add(r.ipa.L[j], bn.GEN)
            proofs[i] = r.serialize()
            err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q,
                                 opp.rounds, 16, zkat.RangeProof.deserialize(proofs[i]))
            assert err is not None
            exp[i] = fts_gpu.FTS_E_RP_INVALID if "IPA" not in err else fts_gpu.FTS_E_IPA_INVALID
        return pp.stage_range_proofs(proofs, coms), exp

    dense, exp_d = make(9500, range(7, m, 32))   # 16 bad proofs: both 256-groups fail
    sparse, exp_s = make(9600, [301])
    assert [int(x) for x in dense.verify()] == exp_d  # alone: marks the batch dense
    out = {}

    def run(name, b):
        out[name] = ([int(x) for x in b.verify()], b.merged(), _raw_timing_names(b))
    # fts_debug_hold: no pass starts before both batches are queued -> one coalesced pass
    pp.hold(2)
    th = [threading.Thread(target=run, args=("d", dense)), threading.Thread(target=run, args=("s", sparse))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert out["d"][0] == exp_d
    assert out["s"][0] == exp_s
    assert out["d"][1] == 2 and out["s"][1] == 2, (out["d"][1], out["s"][1])  # one coalesced pass
    names, work = out["s"][2]
    assert "fb:k_rlc_group_columns" in names and "fb:k_rlc_group_cols" in names, names  # both group sizes ran
    per_proof = work["fb:k_rp_terms_fixed"] / ((3 + 2 * 16) * 15 * 11 * 136)
    assert 1 <= round(per_proof) <= 16 * 8 + 256, per_proof
    for b in (dense, sparse):
        b.close()
    pp.close()


@pytest.mark.gpu
def test_idle_burst_splits_into_even_passes(pp_raw):
    """The dispatcher's idle window (api_rp.cpp fts_rp_batch_verify): 20 batches
    submitted together on an idle device form two passes of 10 (the first pass
    stops at gather_target = coalesce_max / 2 proofs), whatever the submitter
    threads' timing; every caller keeps its own verdicts."""
    import os
    import threading

    import fts_gpu

    m, nb = 64, 20
    # FTS_IDLE_FIRST_US: the first arrival's lone window spans the threads' release too
    # (the default 80 us is measured by bench.py, not asserted here)
    env = dict(FTS_COALESCE_MAX=str(20 * m), FTS_IDLE_GATHER_US="50000", FTS_IDLE_QUIET_US="5000",
               FTS_IDLE_FIRST_US="50000")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pp = fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    rng = random.Random(0x1D1E)
    batches, expect = [], []
    for t in range(nb):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=12000 + t)
        exp = [0] * m
        if t == 7:
            r = zkat.RangeProof.deserialize(proofs[5])
            r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
            proofs[5] = r.serialize()
            exp[5] = fts_gpu.FTS_E_RP_INVALID
        batches.append(pp.stage_range_proofs(proofs, coms))
        expect.append(exp)
    for rep in range(2):
        out, merged = [None] * nb, [0] * nb
        gate = threading.Barrier(nb)

        def run(t):
            gate.wait()
            out[t] = [int(s) for s in batches[t].verify()]
            merged[t] = batches[t].merged()
        th = [threading.Thread(target=run, args=(t,)) for t in range(nb)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert out == expect
        assert merged == [10] * nb, merged
    for b in batches:
        b.close()
    pp.close()


@pytest.mark.gpu
def test_single_fault_locator(pp_raw):
    """api_rp.cpp rp_locate_single / rp_rlc.hip k_rlc_locate: a failed batch
    check with ONE bad proof is decided by the index-weighted recombination
    (S' = (i + 1) S) and that proof's per-proof equations, without the group test;
    the other proofs' deferred IPA structural verdicts (a truncated IPA: "invalid
    IPA proof") still become final.  Two bad proofs: the locator misses, the group
    test decides, and that batch's next failing pass skips the locator (another
    batch's does not).  FTS_LOCATE=0: group
    test only.  Every verdict is the oracle's (bulletproof.go:314-324, ipa.go:195-259)."""
    import os

    import fts_gpu
    from oracle import pp as oppm

    opp = oppm.load_pp(pp_raw).with_bit_length(16)
    status_of = {None: 0, "invalid range proof": 3, "invalid IPA": 6, "invalid IPA proof": 5}

    def ctx(**env):
        env = {k: str(v) for k, v in dict(FTS_LANES="1", FTS_IDLE_GATHER_US="0", **env).items()}
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fts_gpu.PublicParams(pp_raw, bit_length=16, device=0)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    rng = random.Random(0x51F0)
    m = 640

    def batch(pp, bad, seed):
        vals = [rng.getrandbits(16) for _ in range(m)]
        bfs = [rng.randrange(bn.R).to_bytes(32, "big") for _ in range(m)]
        proofs, coms = pp.prove_range_batch_gpu(vals, bfs, seed=seed)
        for i, kind in bad.items():
            r = zkat.RangeProof.deserialize(proofs[i])
            if kind == "T1":
                r.data.T1 = bn.g1_add(r.data.T1, bn.GEN)
            elif kind == "L":
                r.ipa.L[1] = bn.g1_add(r.ipa.L[1], bn.GEN)
            else:  # "short": one IPA round missing (a deferred structural verdict)
                r.ipa.L, r.ipa.R = r.ipa.L[:2], r.ipa.R[:2]
            proofs[i] = r.serialize()
        exp = [0] * m
        for i in bad:
            err = zkat.rp_verify(bn.g1_from_bytes(coms[i]), opp.ped[1:], opp.left, opp.right, opp.P, opp.Q,
                                 opp.rounds, 16, zkat.RangeProof.deserialize(proofs[i]))
            exp[i] = status_of[err]
        return pp.stage_range_proofs(proofs, coms), exp

    def run(b):
        st = [int(x) for x in b.verify()]
        names, _ = _raw_timing_names(b)
        return st, names

    pp = ctx()
    try:
        for bad in ({333: "T1", 17: "short"}, {0: "L"}, {m - 1: "T1"}):
            b, exp = batch(pp, bad, 0x51F1 + len(bad))
            st, names = run(b)
            assert st == exp, {i: (st[i], exp[i]) for i in range(m) if st[i] != exp[i]}
            assert "fb:k_rlc_locate" in names and "fb:k_rlc_group_final" not in names, names
            b.close()
        # two bad proofs in one 256-group: the locator misses, the group test decides
        b2, exp2 = batch(pp, {5: "T1", 100: "L"}, 0x51F9)
        st, names = run(b2)
        assert st == exp2 and "fb:k_rlc_locate" in names and "fb:k_rlc_group_final" in names, names
        # the batch that missed skips the locator in its next failing passes
        # (fts_rp_batch::locate_skip; still sparse: its bad proofs share one 256-group)
        st, names = run(b2)
        assert st == exp2 and "fb:k_rlc_locate" not in names and "fb:k_rlc_group_final" in names, names
        # ... while another caller's single fault still gets the locator (the
        # backoff is per caller batch, not per context)
        b3, exp3 = batch(pp, {222: "L"}, 0x51FB)
        st, names = run(b3)
        assert st == exp3 and "fb:k_rlc_locate" in names and "fb:k_rlc_group_final" not in names, names
        b3.close()
        b2.close()
    finally:
        pp.close()
    pp = ctx(FTS_LOCATE=0)
    try:
        b, exp = batch(pp, {100: "T1"}, 0x51FA)
        st, names = run(b)
        assert st == exp and "fb:k_rlc_locate" not in names and "fb:k_rlc_group_final" in names, names
        b.close()
    finally:
        pp.close()
