"""Audit-info matching on the device (fts_idemix_audit_match_batch, k_idv_audit):
kernel and call time of N items per call on each curve.  Usage:
    python tools/audit_match_bench.py [--items 65536] [--reps 5] [--warmup 2] [--out profiles/audit_match.json]

Inputs: the fixture identities (tests/golden/idemix_audit_golden.json, those that
reach the device) tiled over N items, each item with DISTINCT random (eid, r_eid, rh,
r_rh): repeated scalars would gather the same table rows from cache.
With random openings every verdict is "eid nym does not match"; the kernel has no
early exit on a mismatch, so a lane does the work of a match (hash, two fixed-base
products, the projective comparison) and both halves of every identity run.  The tool
asserts that every status is FTS_E_AUDIT_EID_MISMATCH and says so in its output.

Kernel time: fts_idemix_audit_last_timings (HIP events around the kernel).  Call
time: a host clock around the synchronising C call, the item array built beforehand
(a Go caller hands its slices over the same way)."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))

from fts_gpu import _lib as L  # noqa: E402
from fts_gpu import idemix as I  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def run(tag, d, n, reps, warmup):
    with open(os.path.join(GOLD, "idemix", d["issuer"], "IssuerPublicKey"), "rb") as f:
        V = I.IdentityVerifier(f.read(), device=0, curve=d["curve_id"])
    ids = [bytes.fromhex(c["identity"]) for c in d["cases"]
           if c["error"] is None or c["error"].endswith("does not match")]
    rng = random.Random(0xA0D17 + d["curve_id"])
    keep, items = [], (L.AuditItem * n)()
    for i in range(n):
        ident = ids[i % len(ids)]
        eid = b"user%d.%x" % (i, rng.getrandbits(64))
        rh = b"%d" % rng.getrandbits(40)
        r_eid, r_rh = rng.getrandbits(256).to_bytes(32, "big"), rng.getrandbits(256).to_bytes(32, "big")
        keep.append((ident, eid, rh, r_eid, r_rh))
        it = items[i]
        it.id, it.id_len = C.cast(C.c_char_p(ident), C.c_void_p), len(ident)
        it.eid, it.eid_len = C.cast(C.c_char_p(eid), C.c_void_p), len(eid)
        it.rh, it.rh_len = C.cast(C.c_char_p(rh), C.c_void_p), len(rh)
        it.r_eid32, it.r_rh32 = C.cast(C.c_char_p(r_eid), C.c_void_p), C.cast(C.c_char_p(r_rh), C.c_void_p)
    st = (C.c_int32 * n)()
    kernel, call = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        L.check("fts_idemix_audit_match_batch", L.lib.fts_idemix_audit_match_batch(V.h, n, items, st))
        dt = (time.perf_counter() - t0) * 1e3
        assert all(s == I.FTS_E_AUDIT_EID_MISMATCH for s in st), "a status other than EID_MISMATCH"
        if k >= warmup:
            call.append(dt)
            kernel.append(V.last_audit_kernel_ms())
    V.close()
    km, cm = min(kernel), min(call)
    return {"items": n, "distinct_identities": len(ids), "reps": reps, "warmup": warmup,
            "kernel_ms": [round(x, 4) for x in kernel], "call_ms": [round(x, 3) for x in call],
            "kernel_ms_min": round(km, 4), "call_ms_min": round(cm, 3),
            "kernel_ns_per_identity": round(km * 1e6 / n, 2), "call_ns_per_identity": round(cm * 1e6 / n, 2),
            "identities_per_s_kernel": round(n / km * 1e3, 1), "identities_per_s_call": round(n / cm * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_match.json"))
    a = ap.parse_args()
    with open(os.path.join(GOLD, "idemix_audit_golden.json")) as f:
        doc = json.load(f)
    res = {"tool": "tools/audit_match_bench.py",
           "inputs": "fixture identities tiled, distinct random (eid, r_eid, rh, r_rh) per item: every verdict is "
                     "FTS_E_AUDIT_EID_MISMATCH (asserted); no early exit in the kernel, so the work is a match's",
           "work_per_identity": "2 SHA-256 strings, 4 fixed-base products (<= 64 mixed additions), 2 projective compares"}
    for tag in ("bn254", "fp256bn"):
        res[tag] = run(tag, doc[tag], a.items, a.reps, a.warmup)
        print(tag, json.dumps(res[tag]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
