"""Host cost of an action call's staging (host/action_stage.hpp): DER parse of
N 2-in/2-out transfers straight into the device layout, on a host-only context
(no GPU; fts_debug_stage_actions).  Usage:
    python tools/host_parse_bench.py [N] [bits] [reps]
Prints the mean wall ms per call and the host-thread microseconds per transfer."""
import ctypes as C
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))

import fts_gpu  # noqa: E402
from fts_gpu import _lib as L  # noqa: E402

R_ORDER = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    with open(os.path.join(ROOT, "tests", "golden", "zkatdlog_pp.json"), "rb") as f:
        raw = f.read()
    pp = fts_gpu.PublicParams(raw, bit_length=bits, device=fts_gpu.FTS_DEVICE_NONE)
    rng = random.Random(7)
    T = b"ABC"
    t0 = time.time()
    base = []
    for i in range(min(n, 64)):
        a, b = rng.getrandbits(bits - 2), rng.getrandbits(bits - 2)
        c = rng.randrange(a + b + 1)
        ib = [rng.randrange(R_ORDER).to_bytes(32, "big") for _ in range(2)]
        ob = [rng.randrange(R_ORDER).to_bytes(32, "big") for _ in range(2)]
        ins = [pp.token_commit(T, v, x) for v, x in zip([a, b], ib)]
        outs = [pp.token_commit(T, v, x) for v, x in zip([c, a + b - c], ob)]
        base.append((ins, outs, pp.prove_transfer(T, [a, b], ib, [c, a + b - c], ob, 1000 + i)))
    prove_s = time.time() - t0
    batch = pp.prepare_transfers([base[i % len(base)] for i in range(n)])
    # the fastest of `reps` calls of 3 repetitions each (a shared host's noise only adds)
    ms, best = (C.c_float * 4)(), None
    for _ in range(reps):
        L.check("fts_debug_stage_actions", L.lib.fts_debug_stage_actions(pp._ctx, n, batch.items, 0, None, 3, ms))
        if best is None or ms[0] < best[0]:
            best = list(ms)
    ms = best
    thr = min(16, os.cpu_count() or 1)
    print({"transfers": n, "bits": bits, "reps": reps, "ms_per_call": round(ms[0], 3),
           "ms_steps": [round(x, 3) for x in ms[1:]],
           "us_per_transfer_wall": round(ms[0] * 1e3 / n, 3),
           "host_threads": thr, "us_per_transfer_thread": round(ms[0] * 1e3 * thr / n, 3),
           "prove_s": round(prove_s, 1)})


if __name__ == "__main__":
    main()
