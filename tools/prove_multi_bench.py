"""Generation on a multi-device context: single-device no-regression and scaling.
    python tools/prove_multi_bench.py [--parent-lib PATH/libfts_gpu.so] [--out profiles/prove_multi.json]

Workload: 8,192 2-in/2-out 64-bit transfers per fts_transfer_generate_batch_gpu call, 3
calls in flight, 2 warm-up and 5 timed rounds of 3 calls (tools/generate_bench.py's
generation shape).  Arms, two processes each, alternating:

  single         devices [0] (a single-device context) on this build
  parent         the same on --parent-lib (a build of the parent commit, through FTS_LIB)
  multi_*        with more than one device: [0, 1], and all devices if there are more;
                 with one device: [0, 0] (two shards on one card: the split, thread and
                 merge code, no gain expected)

Recorded: every round's rate; the parent's own run-to-run spread and whether this
build's [0] median lies inside it; the ratio of each multi arm to [0]; and per child
of the context its fts_debug_shard_work counters and the host phases of its last pass
(host_prep_ms: randomness staged, host_wait_ms: device, host_parse_ms: DER) from
fts_debug_shard_timings -- the host share per device is what says at which device count
the one host pool binds.

Each measurement is a child process (`--mode run`) that prints one JSON line; a child
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


def _witnesses(n, seed):
    """n 2-in/2-out transfers (type, inputs, outputs); input commitments are not checked
    by the generators: any 64 bytes of the right shape"""
    rng = random.Random(seed)
    gen = []
    for i in range(n):
        iv = [rng.randrange(1 << 62), rng.randrange(1 << 62)]
        o0 = rng.randrange(iv[0] + iv[1])
        ins = [(b"tx-%d" % i, k, b"alice", bytes(64), v, rng.randrange(R).to_bytes(32, "big"))
               for k, v in enumerate(iv)]
        gen.append((b"ABC", ins, [(o0, b"bob"), (iv[0] + iv[1] - o0, b"bob")]))
    return gen


def mode_run(a):
    import fts_gpu as F
    import fts_gpu._lib as L
    devices = [int(d) for d in a.devices.split(",")]
    with open(PP, "rb") as f:
        raw = f.read()
    # [0]: the single-device context itself (what the parent build is compared on)
    pp = F.PublicParams(raw, bit_length=64, device=devices[0]) if len(devices) == 1 else \
        F.PublicParams(raw, bit_length=64, devices=devices)
    gen = _witnesses(a.actions, 1)
    batches = [F.GenBatch([(t, i, o, b"") for t, i, o in gen], pp.rounds) for _ in range(a.inflight)]
    out = {}

    def call(j):
        out[j] = pp.generate_transfers_gpu(batches[j], seed=1000 + j * a.actions)
    rates = []
    with ThreadPoolExecutor(a.inflight) as ex:
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            list(ex.map(call, range(a.inflight)))
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                rates.append(a.inflight * a.actions / dt)
    req = F.request.token_request([(F.request.TRANSFER, out[0][0][0])], [b"sig"])
    d = {"devices": devices, "lib": os.path.relpath(L.LIB_PATH, ROOT), "actions_per_call": a.actions, "inflight": a.inflight,
         "actions_per_s": [round(r, 1) for r in rates], "median": round(sorted(rates)[len(rates) // 2], 1),
         "min": round(min(rates), 1), "max": round(max(rates), 1),
         "first_action_inspect": F.inspect_request(req)["status"]}
    if hasattr(L.lib, "fts_debug_shard_work"):  # not in a parent build
        d["shards"] = []
        for j in range(len(devices)):
            t = pp.shard_timings(j)
            w = pp.shard_work(j)
            d["shards"].append({"device": devices[j], "range_proofs": w[0], "actions": w[1], "tokens": w[2],
                                "passes": w[3], "host_prep_ms": round(t.get("host_prep", 0.0), 3),
                                "host_parse_ms": round(t.get("host_parse", 0.0), 3),
                                "host_wait_ms": round(t.get("host_wait_flag", 0.0), 3)})
    print(json.dumps(d))


def child(devices, env, fwd):
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "run", "--devices", devices, *fwd],
                         env=e, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("prove_multi_bench: child [%s] failed (%d); nothing more is started" % (devices, out.returncode))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    print("[%s]" % devices, "parent" if env else "new", line, flush=True)
    return json.loads(line)


def _all_rates(runs):
    return [r for run in runs for r in run["actions_per_s"]]


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all", "run"])
    ap.add_argument("--devices", default="0")
    ap.add_argument("--actions", type=int, default=8192)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_multi.json"))
    a = ap.parse_args()
    if a.mode == "run":
        return mode_run(a)
    # counted in a child: this process only starts children and never opens a device
    ndev = int(subprocess.check_output([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"],
                                       text=True, timeout=300).split()[-1])
    fwd = ["--actions", str(a.actions), "--inflight", str(a.inflight), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    parent = {"FTS_LIB": os.path.abspath(a.parent_lib)} if a.parent_lib else None
    if ndev > 1:
        multi = ["0,1"] + ([",".join(str(d) for d in range(ndev))] if ndev > 2 else [])
    else:
        multi = ["0,0"]
    res = {"tool": "tools/prove_multi_bench.py", "device_count": ndev, "single": [], "parent": [],
           "multi": {m: [] for m in multi}}
    for k in range(2):  # two processes per arm, alternating; the second pass in reverse order
        arms = [("single", "0", None)] + ([("parent", "0", parent)] if parent else []) + [(m, m, None) for m in multi]
        for name, devs, env in (arms if k == 0 else arms[::-1]):
            (res["multi"][name] if name in res["multi"] else res[name]).append(child(devs, env, fwd))
    s = _all_rates(res["single"])
    summ = {"single_median": _median(s), "single_spread": [min(s), max(s)],
            "single_process_medians": [r["median"] for r in res["single"]]}
    if parent:
        p = _all_rates(res["parent"])
        summ.update({"parent_median": _median(p), "parent_spread": [min(p), max(p)],
                     "parent_process_medians": [r["median"] for r in res["parent"]],
                     "single_median_inside_parent_spread": min(p) <= _median(s) <= max(p),
                     "single_over_parent": round(_median(s) / _median(p), 4)})
    for m in multi:
        r = _all_rates(res["multi"][m])
        summ["multi_%s_median" % m] = _median(r)
        summ["multi_%s_over_single" % m] = round(_median(r) / _median(s), 4)
    if ndev < 2:
        summ["note"] = "one device: [0, 0] puts two shards on one card; scaling over cards is unmeasured"
    res["summary"] = summ
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summ))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
