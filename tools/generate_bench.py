"""Token commitments and whole-action generation on the device: kernel and call rates.
    python tools/generate_bench.py [--parent-lib PATH/libfts_gpu.so] [--out profiles/generate.json]

Commit kernel (fts_token_commit_batch_gpu, k_token_commit): HIP-event time per 65,536
tokens with DISTINCT random (value, bf) per item -- repeated scalars would gather the
same table rows from cache -- against k_open_check on the same tokens in
the same process (64-bit values, 256-bit blinding factors on both sides), for 1 / 2 / 4 /
8 / 16 tokens per lane (FTS_COMMIT_PER_LANE, one process each), and again at 2^20 tokens
(--big-tokens), where one token per lane is 16 waves per SIMD.

Generation (fts_transfer_generate_batch_gpu): 8,192 2-in/2-out transfers at 64 bits per
call, 3 calls in flight, 2 warm-up and 5 timed rounds of 3 calls.  Baseline: what a caller
did before the generators existed, on the same witnesses: fts_transfer_prove_batch_gpu,
fts_token_commit for every output on 16 host threads, the Python writers of
fts_gpu.request -- run against --parent-lib (a build of the parent commit, through
FTS_LIB) when given, processes alternating.  Prove-only rates of both builds beside it.

Each measurement is a child process (`--mode ...`) that prints one JSON line; a child
that fails ends the run."""
import argparse
import json
import os
import random
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
PP = os.path.join(ROOT, "tests", "golden", "zkatdlog_pp.json")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def _ctx(bits):
    import fts_gpu
    with open(PP, "rb") as f:
        return fts_gpu, fts_gpu.PublicParams(f.read(), bit_length=bits, device=0)


def mode_commit(a):
    F, pp = _ctx(64)
    rng = random.Random(0xC0117)
    n = a.tokens
    types = [b"ABC", b"USD", b"EUR", b"a-longer-token-type-name"]
    items = [(types[i & 3], rng.getrandbits(64), rng.getrandbits(256).to_bytes(32, "big")) for i in range(n)]
    kc, ko, coms = [], [], None
    for k in range(a.warmup + a.reps):
        coms = pp.token_commit_batch_gpu(items)
        t = pp.last_timings()["k_token_commit"]
        if k >= a.warmup:
            kc.append(t)
    ob = pp.prepare_openings([(c, t, v.to_bytes(32, "big"), b) for c, (t, v, b) in zip(coms, items)])
    for k in range(a.warmup + a.reps):
        st = pp.check_openings(ob)
        assert not st.any(), "a device commitment failed the device opening check"
        t = pp.last_timings()["k_open_check"]
        if k >= a.warmup:
            ko.append(t)
    sample = [0, 1, n // 2, n - 1]
    assert all(coms[i] == pp.token_commit(*items[i]) for i in sample), "device commitment != fts_token_commit"
    print(json.dumps({"tokens": n, "tokens_per_lane": F.token_commit_batch_width() // 64,
                      "k_token_commit_ms": [round(x, 4) for x in kc], "k_open_check_ms": [round(x, 4) for x in ko],
                      "k_token_commit_ms_min": round(min(kc), 4), "k_open_check_ms_min": round(min(ko), 4),
                      "ratio_commit_over_open": round(min(kc) / min(ko), 4)}))


def _witnesses(pp, n, seed):
    """n 2-in/2-out transfers: (type, inputs, outputs) for the generators, and the same
    witnesses as the provers take them (output blinding factors drawn by the caller)"""
    rng = random.Random(seed)
    gen, wit = [], []
    for i in range(n):
        iv = [rng.randrange(1 << 62), rng.randrange(1 << 62)]
        o0 = rng.randrange(iv[0] + iv[1])
        ov = [o0, iv[0] + iv[1] - o0]
        ib = [rng.randrange(R).to_bytes(32, "big") for _ in iv]
        ob = [rng.randrange(R).to_bytes(32, "big") for _ in ov]
        # input commitments are not checked by either path: any 64 bytes of the right shape
        ins = [(b"tx-%d" % i, k, b"alice", bytes(64), v, b) for k, (v, b) in enumerate(zip(iv, ib))]
        gen.append((b"ABC", ins, [(v, b"bob") for v in ov]))
        wit.append((b"ABC", iv, ib, ov, ob))
    return gen, wit


def _rounds(a, one_call):
    """a.inflight concurrent calls per round; warm-up rounds, then timed ones -> actions/s per round"""
    rates = []
    with ThreadPoolExecutor(a.inflight) as ex:
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            list(ex.map(one_call, range(a.inflight)))
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                rates.append(a.inflight * a.actions / dt)
    return rates


def _report(a, what, rates, extra=None):
    import fts_gpu._lib as L
    d = {"what": what, "lib": L.LIB_PATH, "actions_per_call": a.actions, "inflight": a.inflight,
         "actions_per_s": [round(r, 1) for r in rates], "median": round(sorted(rates)[len(rates) // 2], 1),
         "min": round(min(rates), 1), "max": round(max(rates), 1)}
    d.update(extra or {})
    print(json.dumps(d))


def mode_generate(a):
    F, pp = _ctx(64)
    gen, _ = _witnesses(pp, a.actions, 1)
    batches = [F.GenBatch([(t, i, o, b"") for t, i, o in gen], pp.rounds) for _ in range(a.inflight)]
    out = {}

    def call(j):
        out[j] = pp.generate_transfers_gpu(batches[j], seed=1000 + j * a.actions)
    rates = _rounds(a, call)
    # what was timed is a real action: the first one verifies as a request
    req = F.request.token_request([(F.request.TRANSFER, out[0][0][0])], [b"sig"])
    _report(a, "fts_transfer_generate_batch_gpu", rates, {"first_action_inspect": F.inspect_request(req)["status"]})


def mode_baseline(a):
    F, pp = _ctx(64)
    _, wit = _witnesses(pp, a.actions, 1)
    wbs = [F.WitnessBatch(wit, pp.rounds) for _ in range(a.inflight)]
    commit_pool = ThreadPoolExecutor(16)

    def call(j):
        proofs = pp.prove_transfers_gpu(wbs[j], seed=1000 + j * a.actions)
        flat = [(t, v, b) for t, _, _, ov, ob in wit for v, b in zip(ov, ob)]
        coms = list(commit_pool.map(lambda x: pp.token_commit(*x), flat, chunksize=256))
        acts, metas = [], []
        for i, (t, iv, ib, ov, ob) in enumerate(wit):
            ins = [(b"tx-%d" % i, k, b"alice", bytes(64)) for k in range(2)]
            acts.append(F.request.transfer_action(ins, [(b"bob", coms[2 * i]), (b"bob", coms[2 * i + 1])], proofs[i]))
            metas += [F.request.token_metadata(t, v.to_bytes(32, "big"), b) for v, b in zip(ov, ob)]
        return acts, metas
    _report(a, "prove_batch_gpu + token_commit x 16 threads + Python writers", _rounds(a, call))


def mode_prove(a):
    F, pp = _ctx(64)
    _, wit = _witnesses(pp, a.actions, 1)
    wbs = [F.WitnessBatch(wit, pp.rounds) for _ in range(a.inflight)]
    _report(a, "fts_transfer_prove_batch_gpu", _rounds(a, lambda j: pp.prove_transfers_gpu(wbs[j], seed=1000 + j)))


def split_excess(c):
    """per tokens-per-lane e of one batch size: the excess over k_open_check, split into the
    inversions and the rest.  An inversion per token costs I, one per e tokens I / e, so where
    sharing pays (t_e < t_1) I = (t_1 - t_e) / (1 - 1 / e); e = 1 is split with the I of the
    fastest e.  Where t_e >= t_1 the lanes no longer fill the chip and no split is given."""
    if "per_lane_1" not in c:
        return
    t1, t_open = c["per_lane_1"]["k_token_commit_ms_min"], min(v["k_open_check_ms_min"] for v in c.values())
    inv = None
    for k, v in c.items():
        e, te = v["tokens_per_lane"], v["k_token_commit_ms_min"]
        v["excess_over_open_check_ms"] = round(te - t_open, 4)
        if e > 1 and te < t1:
            i_e = (t1 - te) / (1 - 1.0 / e)
            v["inversions_ms"] = round(i_e / e, 4)
            v["rest_of_excess_ms"] = round(te - t_open - i_e / e, 4)
            if inv is None or te < inv[0]:
                inv = (te, i_e)
        elif e > 1:
            v["note"] = "slower than one token per lane: too few waves at this batch size"
    if inv:
        v = c["per_lane_1"]
        v["inversions_ms"] = round(inv[1], 4)
        v["rest_of_excess_ms"] = round(t1 - t_open - inv[1], 4)


def child(mode, env=None, extra=()):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, *extra], env=e,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("generate_bench: child %s failed (%d); nothing more is started" % (mode, out.returncode))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    print(mode, env or "", line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "commit", "generate", "baseline", "prove"])
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--actions", type=int, default=8192)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-tokens", type=int, default=1 << 20, help="second size of the commit A/B (0: skip)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate.json"))
    a = ap.parse_args()
    if a.mode != "all":
        return {"commit": mode_commit, "generate": mode_generate, "baseline": mode_baseline, "prove": mode_prove}[a.mode](a)
    fwd = ["--tokens", str(a.tokens), "--actions", str(a.actions), "--inflight", str(a.inflight), "--reps", str(a.reps),
           "--warmup", str(a.warmup)]
    res = {"tool": "tools/generate_bench.py", "commit": {}, "commit_big": {}, "generation": {}}
    for e in (1, 2, 4, 8, 16):
        res["commit"]["per_lane_%d" % e] = child("commit", {"FTS_COMMIT_PER_LANE": str(e)}, fwd)
    # the same A/B where the chip is full (16 waves per SIMD at one token per lane)
    big = ["--tokens", str(a.big_tokens), "--reps", "3", "--warmup", "1"]
    for e in (1, 2, 4, 8) if a.big_tokens else ():
        res["commit_big"]["per_lane_%d" % e] = child("commit", {"FTS_COMMIT_PER_LANE": str(e)}, big)
    for c in (res["commit"], res["commit_big"]):
        split_excess(c)
    parent = {"FTS_LIB": os.path.abspath(a.parent_lib)} if a.parent_lib else {}
    g = res["generation"]
    g["baseline_is_parent_build"] = bool(a.parent_lib)
    for r in range(2):
        g["generate_run%d" % r] = child("generate", None, fwd)
        g["baseline_run%d" % r] = child("baseline", parent, fwd)
    g["prove_only_new"] = child("prove", None, fwd)
    g["prove_only_parent"] = child("prove", parent, fwd) if a.parent_lib else None
    base = g["baseline_run0"]["actions_per_s"] + g["baseline_run1"]["actions_per_s"]
    gen = g["generate_run0"]["actions_per_s"] + g["generate_run1"]["actions_per_s"]
    g["baseline_spread"] = [min(base), max(base)]
    g["generate_median"], g["baseline_median"] = sorted(gen)[len(gen) // 2], sorted(base)[len(base) // 2]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
