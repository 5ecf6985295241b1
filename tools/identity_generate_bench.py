"""Identity generation on the device: call rate, kernel times and host share of
fts_idemix_identity_generate_batch on both curves, beside fts_idemix_identity_verify_batch on
the identities it produced (the yardstick), in the same run.
    python tools/identity_generate_bench.py [--out profiles/identity_generate.json]

Per curve: 65,536 identities per call, 3 calls in flight (the handle's slots), 2 warm-up and 5
timed rounds of 3 calls, as tools/sign_bench.py.  Rate = identities / host time of a round
(every call ends in a stream synchronise); kernel times are the HIP events of the last call
(k_idg_prep + k_idg_points, k_idg_finish), host times the host pool's draw + staging and
serialisation seconds of that call (fts_idemix_identity_generate_last_timings).  Every call has
its own seed, so every scalar and every table row gathered is distinct.  The identities of the
last round are then verified on the device (every verdict FTS_OK): that gives
fts_idemix_identity_verify_batch's rate and kernel times on the same items.

The MAD share of k_idg_points is computed from its algorithmic count: 23 table walks of 16
windows per identity, each a mixed addition (7 products + 4 squarings = 11 field products
with the Jacobian accumulator of the identity kernels), 136 u32 MADs per Montgomery product
(64 + 64 + 8: the library's cost model), against the 19.66 T MAD/s peak
that tools/pass_mads.py uses.

Each curve is a child process (`--mode ...`) that prints one JSON line; a child that fails
ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "idemix")
CURVES = {"bn254": ("bn254_charlie", 1), "fp256bn": ("fp256bn_validator", 0)}

# k_idg_points per identity: table walks x windows x field products per mixed addition x MADs per product
WALKS, WINDOWS, PRODUCTS_PER_MADD, MADS_PER_PRODUCT = 23, 16, 11, 136
MAD_PEAK_PER_S = 19.661e12


def _med(x):
    return sorted(x)[len(x) // 2]


def _spread(x):
    return {"min": round(min(x), 4), "median": round(_med(x), 4), "max": round(max(x), 4)}


def mode_curve(a):
    import ctypes as C

    import numpy as np
    from fts_gpu import _lib as L, idemix as I
    d, cid = CURVES[a.mode]
    with open(os.path.join(GOLD, d, "IssuerPublicKey"), "rb") as f:
        ipk = f.read()
    with open(os.path.join(GOLD, d, "SignerConfig"), "rb") as f:
        sc = f.read()
    ver = I.IdentityVerifier(ipk, device=0, curve=cid)
    dev = I.Credential.from_signer_config(ver, sc)
    n, ln = a.n, dev.identity_len
    # the C entry point on buffers allocated once per slot (no Python marshaling in the timed region)
    out = [(np.zeros(n * ln, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(32 * n, dtype=np.uint8),
            np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8), np.zeros(n, dtype=np.int32))
           for _ in range(a.inflight)]
    rates, kms, host, walls = [], [], [], []
    with ThreadPoolExecutor(a.inflight) as ex:
        for k in range(a.warmup + a.reps):
            def call(j, k=k):
                ids, lens, rn, re_, rr, st = out[j]
                L.check("fts_idemix_identity_generate_batch",
                        L.lib.fts_idemix_identity_generate_batch(dev.h, n, 1 + (k * a.inflight + j) * n, None, None,
                                                                 ids.ctypes.data, ln, lens.ctypes.data, rn.ctypes.data,
                                                                 re_.ctypes.data, rr.ctypes.data,
                                                                 st.ctypes.data_as(C.POINTER(C.c_int32))))
            t0 = time.perf_counter()
            list(ex.map(call, range(a.inflight)))
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                rates.append(a.inflight * n / dt)
                walls.append(dt)
                t = dev.last_timings()
                kms.append(t[:2])
                host.append(t[2:])
    assert all(not o[5].any() and (o[1] == ln).all() for o in out)
    raw = out[0][0].tobytes()
    vrates, vms = [], []
    prep = ver.prepare([raw[i * ln:(i + 1) * ln] for i in range(n)])
    for k in range(4):  # the first one warms the verify kernels up
        t0 = time.perf_counter()
        st = ver.verify_prepared(prep)
        dt = time.perf_counter() - t0
        assert not st.any(), "a generated identity failed the device verifier"
        if k:
            vrates.append(n / dt)
            vms.append(ver.last_kernel_ms())
    pts_ms = min(v[0] for v in kms)
    mads = WALKS * WINDOWS * PRODUCTS_PER_MADD * MADS_PER_PRODUCT * n
    res = {"what": "fts_idemix_identity_generate_batch " + a.mode, "n_per_call": n, "inflight": a.inflight,
           "identity_len": dev.identity_len,
           "identities_per_s": [round(r, 1) for r in rates], "identities_per_s_median": round(_med(rates), 1),
           "identities_per_s_spread": _spread(rates),
           "kernel_ms": {"k_idg_prep+k_idg_points": _spread([v[0] for v in kms]),
                         "k_idg_finish": _spread([v[1] for v in kms])},
           "kernel_identities_per_s": round(n / ((pts_ms + min(v[1] for v in kms)) * 1e-3), 1),
           "host_s_per_call": {"draw_and_stage": _spread([h[0] for h in host]),
                               "serialise": _spread([h[1] for h in host])},
           # a call's host-pool seconds over the round's wall time (the calls of a round share the pool)
           "host_share_of_round": round(a.inflight * _med([h[0] + h[1] for h in host]) / _med(walls), 4),
           "k_idg_points_mads_per_identity": WALKS * WINDOWS * PRODUCTS_PER_MADD * MADS_PER_PRODUCT,
           "k_idg_points_mad_share_of_peak": round(mads / (pts_ms * 1e-3) / MAD_PEAK_PER_S, 4),
           "verify_identities_per_s": _spread(vrates),
           "verify_kernel_ms": {"tvals": _spread([v[0] for v in vms]), "pairing": _spread([v[1] for v in vms])},
           "generate_over_verify_rate": round(_med(rates) / _med(vrates), 4)}
    print(json.dumps(res))
    dev.close()
    ver.close()


def child(mode, extra):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, *extra], capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("identity_generate_bench: child %s failed (%d); nothing more is started" % (mode, out.returncode))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    print(mode, line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all"] + list(CURVES))
    ap.add_argument("--n", type=int, default=65536)  # four tiles of 16,384 per call
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_generate.json"))
    a = ap.parse_args()
    if a.mode != "all":
        return mode_curve(a)
    fwd = ["--n", str(a.n), "--inflight", str(a.inflight), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    res = {"tool": "tools/identity_generate_bench.py", "runs": {m: child(m, fwd) for m in CURVES}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
