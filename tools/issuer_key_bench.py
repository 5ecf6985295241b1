"""Idemix issuer keys on the device: the HIP-event time of one fts_idemix_ipk_check_batch call and
of one fts_idemix_issuer_keygen_batch call at n = 1 and n = 64 keys, on both curves.
    python tools/issuer_key_bench.py [--out profiles/issuer_key.json]

Both calls run one lane per key when a key is imported or made, never in bulk: the figures
are latencies of a mostly empty device (n = 64 is one wave), not rates.  Per (curve, n): 2
warm-up calls and 9 timed ones, one at a time; the kernel time is the call's own HIP events
(fts_idemix_issuer_key_last_timings: the kernel sequence without the copies), the wall time
the host clock around the whole call, which ends in a stream synchronise and includes the
call's stream, event and buffer allocations.  The keys checked are the ones the keygen call
made (every verdict FTS_OK)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
CURVES = {"bn254": 1, "fp256bn": 0}


def _spread(x):
    return {"min": round(min(x), 4), "median": round(sorted(x)[len(x) // 2], 4), "max": round(max(x), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "issuer_key.json"))
    a = ap.parse_args()
    from fts_gpu import idemix as I
    runs = {}
    for tag, cid in CURVES.items():
        for n in (1, 64):
            gen_ms, gen_wall, chk_ms, chk_wall = [], [], [], []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                keys = I.generate_issuer_keys(n, cid, seed=1000 * (k + 1))
                t1 = time.perf_counter()
                g = I.issuer_key_last_kernel_ms()[1]
                ipks = [ipk for _, ipk in keys]
                t2 = time.perf_counter()
                st = I.check_issuer_keys(ipks, cid)
                t3 = time.perf_counter()
                c = I.issuer_key_last_kernel_ms()[0]
                assert not st.any(), "a generated key failed the check"
                if k >= a.warmup:
                    gen_ms.append(g), gen_wall.append(1e3 * (t1 - t0)), chk_ms.append(c), chk_wall.append(1e3 * (t3 - t2))
            runs["%s_n%d" % (tag, n)] = {"keygen_kernel_ms": _spread(gen_ms), "keygen_call_ms": _spread(gen_wall),
                                         "check_kernel_ms": _spread(chk_ms), "check_call_ms": _spread(chk_wall)}
            print(tag, n, json.dumps(runs["%s_n%d" % (tag, n)]), flush=True)
    res = {"tool": "tools/issuer_key_bench.py", "reps": a.reps, "warmup": a.warmup, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
