"""Idemix enrolment on the device: call rates, kernel times and host share of
fts_idemix_cred_request_batch, fts_idemix_cred_request_verify_batch and
fts_idemix_cred_issue_batch on both curves, in one run.
    python tools/cred_issue_bench.py [--out profiles/cred_issue.json]

Per curve: 65,536 items per call, 3 calls in flight (the handle's slots), 2 warm-up and 5 timed
rounds of 3 calls, as tools/identity_generate_bench.py.  Rate = items / host time of a round
(every call ends in a stream synchronise); kernel times are the HIP events of the last call;
host times the host pool's parse + draw + staging and serialisation seconds of that call
(fts_idemix_cred_issue_last_timings).  With three calls in flight a call's events include the
time its kernels wait behind the other two streams', so the issue call is then timed alone as
well (`alone`: one call in flight, the same rounds): those kernel times are the device's.
Every call has its own seed.  BN254 runs under bn254_tokengen (the reference's own issuer
secret), FP256BN under a key made by tests/cred_issue_ref.py make_issuer_key.  The requests the issuer is timed on are the ones the
request call made; 256 of the issued credentials are then verified on the device (FTS_OK).

The products' share of the MAD peak is computed from their algorithmic count per credential:
six fixed-base walks of 16 windows, each a mixed addition of 11 field products, and two GLV
chains (c Nym, inv B) of 124 doublings of 7 field products and 64 mixed additions (an upper
bound: one digit in sixteen is zero; the lane tables' build and the inversions are not
counted), 136 u32 MADs per Montgomery product (the library's cost model),
against the 19.66 T MAD/s peak that tools/pass_mads.py uses: over a round of three calls in
flight (`..._in_round`, what the device sustains) and over the kernels of a call alone.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
CURVES = ("bn254", "fp256bn")

FIXED_WALKS, WINDOWS, PRODUCTS_PER_MADD, PRODUCTS_PER_DBL, MADS_PER_PRODUCT = 6, 16, 11, 7, 136
GLV_CHAINS, GLV_DBL, GLV_MADD = 2, 124, 64
PRODUCTS_PER_CRED = FIXED_WALKS * WINDOWS * PRODUCTS_PER_MADD + \
    GLV_CHAINS * (GLV_DBL * PRODUCTS_PER_DBL + GLV_MADD * PRODUCTS_PER_MADD)
MAD_PEAK_PER_S = 19.661e12


def _med(x):
    return sorted(x)[len(x) // 2]


def _spread(x):
    return {"min": round(min(x), 4), "median": round(_med(x), 4), "max": round(max(x), 4)}


def mode_curve(a):
    import ctypes as C
    import random

    import numpy as np
    import cred_issue_ref as R
    from fts_gpu import _lib as L, idemix as I
    cid = R.CURVES[a.mode][0]
    isk, ipk = R.tokengen() if a.mode == "bn254" else R.make_issuer_key(a.mode, random.Random(4100))
    ver = I.IdentityVerifier(ipk, device=0, curve=cid)
    iss = I.Issuer(ver, isk)
    n, RL, CL = a.n, I.FTS_IDEMIX_CRED_REQUEST_LEN, I.FTS_IDEMIX_CREDENTIAL_LEN
    rs = np.random.RandomState(5)
    sk = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    sk[:, 0] = 0  # below either r
    nonce = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    attrs = rs.randint(0, 256, size=(n, 4, 32), dtype=np.uint8)
    attrs[:, :, 0] = 0
    i32p = C.POINTER(C.c_int32)
    # the C entry points on buffers allocated once per slot (no Python marshaling in the timed region)
    slot = [{"req": np.zeros(n * RL, dtype=np.uint8), "cred": np.zeros(n * CL, dtype=np.uint8),
             "len": np.zeros(n, dtype=np.uint32), "st": np.zeros(n, dtype=np.int32)} for _ in range(a.inflight)]
    for s in slot:
        s["ritems"] = np.zeros(n, dtype=[("req", "u8"), ("req_len", "u8")])
        s["ritems"]["req"] = s["req"].ctypes.data + RL * np.arange(n, dtype=np.uint64)
        s["ritems"]["req_len"] = RL
        s["iitems"] = np.zeros(n, dtype=[("req", "u8"), ("req_len", "u8"), ("attrs", "u8")])
        s["iitems"]["req"], s["iitems"]["req_len"] = s["ritems"]["req"], RL
        s["iitems"]["attrs"] = attrs.ctypes.data + 128 * np.arange(n, dtype=np.uint64)

    def rounds(call, timings, inflight=a.inflight):
        rates, walls, tm = [], [], []
        with ThreadPoolExecutor(inflight) as ex:
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                list(ex.map(lambda j, k=k: call(j, 1 + (k * inflight + j) * n), range(inflight)))
                dt = time.perf_counter() - t0
                if k >= a.warmup:
                    rates.append(inflight * n / dt)
                    walls.append(dt)
                    tm.append(timings())
                assert all(not s["st"].any() for s in slot)
        return rates, walls, tm

    def make(j, seed):
        s = slot[j]
        L.check("fts_idemix_cred_request_batch",
                L.lib.fts_idemix_cred_request_batch(ver.h, n, sk.ctypes.data, nonce.ctypes.data, seed, s["req"].ctypes.data,
                                                    RL, s["len"].ctypes.data, s["st"].ctypes.data_as(i32p)))

    def check(j, seed):
        s = slot[j]
        L.check("fts_idemix_cred_request_verify_batch",
                L.lib.fts_idemix_cred_request_verify_batch(ver.h, n, C.cast(s["ritems"].ctypes.data, C.POINTER(L.CredReqItem)),
                                                           s["st"].ctypes.data_as(i32p)))

    def issue(j, seed):
        s = slot[j]
        L.check("fts_idemix_cred_issue_batch",
                L.lib.fts_idemix_cred_issue_batch(iss.h, n, C.cast(s["iitems"].ctypes.data, C.POINTER(L.CredIssueItem)),
                                                  seed, s["cred"].ctypes.data, CL, s["len"].ctypes.data,
                                                  s["st"].ctypes.data_as(i32p)))

    mk_rates, _, mk_ms = rounds(make, lambda: ver.last_cred_request_kernel_ms()[0])
    ck_rates, _, ck_ms = rounds(check, lambda: ver.last_cred_request_kernel_ms()[1])
    is_rates, walls, is_tm = rounds(issue, iss.last_timings)
    one_rates, one_walls, one_tm = rounds(issue, iss.last_timings, inflight=1)
    assert all((s["len"] == CL).all() for s in slot)
    raw = slot[0]["cred"].tobytes()
    st = ver.verify_credentials([raw[i * CL:(i + 1) * CL] for i in range(256)], [sk[i].tobytes() for i in range(256)])
    assert not st.any(), "an issued credential failed the device verifier"
    kern = [t[0] + t[1] for t in is_tm]
    host = [t[2] + t[3] for t in is_tm]
    one_kern = [t[0] + t[1] for t in one_tm]
    one_host = [t[2] + t[3] for t in one_tm]
    mads = PRODUCTS_PER_CRED * MADS_PER_PRODUCT
    res = {"what": "fts_idemix_cred_issue_batch " + a.mode, "n_per_call": n, "inflight": a.inflight,
           "request_len": RL, "credential_len": CL,
           "credentials_per_s": [round(r, 1) for r in is_rates], "credentials_per_s_median": round(_med(is_rates), 1),
           "credentials_per_s_spread": _spread(is_rates),
           "requests_made_per_s": _spread(mk_rates), "requests_verified_per_s": _spread(ck_rates),
           "kernel_ms": {"k_ci_decode+k_ci_var+k_ci_check": _spread([t[0] for t in is_tm]),
                         "k_ci_sign": _spread([t[1] for t in is_tm]),
                         "k_ci_request": _spread(mk_ms), "request_verify": _spread(ck_ms)},
           # (a call's events with two other calls' kernels on the device: not the device's own time)
           "host_s_per_call": {"parse_draw_and_stage": _spread([t[2] for t in is_tm]),
                               "serialise": _spread([t[3] for t in is_tm])},
           # a call's host-pool seconds over the round's wall time (the calls of a round share the pool)
           "host_share_of_round": round(a.inflight * _med(host) / _med(walls), 4),
           "alone": {"credentials_per_s": _spread(one_rates),
                     "kernel_ms": {"k_ci_decode+k_ci_var+k_ci_check": _spread([t[0] for t in one_tm]),
                                   "k_ci_sign": _spread([t[1] for t in one_tm])},
                     "kernel_credentials_per_s": round(n / (min(one_kern) * 1e-3), 1),
                     "host_s_per_call": _spread(one_host),
                     # of one call's wall time: its kernels, its host-pool seconds (the rest: copies, launches)
                     "kernel_share_of_call": round(_med(one_kern) * 1e-3 / _med(one_walls), 4),
                     "host_share_of_call": round(_med(one_host) / _med(one_walls), 4)},
           "product_mads_per_credential": mads,
           "product_mad_share_of_peak_in_round": round(mads * _med(is_rates) / MAD_PEAK_PER_S, 4),
           "product_mad_share_of_peak_alone": round(mads * n / (min(one_kern) * 1e-3) / MAD_PEAK_PER_S, 4)}
    print(json.dumps(res))
    iss.close()
    ver.close()


def child(mode, extra):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, *extra], capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("cred_issue_bench: child %s failed (%d); nothing more is started" % (mode, out.returncode))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cred_issue.json"))
    a = ap.parse_args()
    if a.mode != "all":
        return mode_curve(a)
    fwd = ["--n", str(a.n), "--inflight", str(a.inflight), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    res = {"tool": "tools/cred_issue_bench.py", "runs": {m: child(m, fwd) for m in CURVES}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
