"""Signing on the device: call rates and kernel times of fts_ecdsa_sign_batch (both nonce
modes) and fts_nym_sign_batch (both curves), beside the verify kernels at the same n.
    python tools/sign_bench.py [--out profiles/sign.json]

Per configuration: 65,536 signatures per call, 3 calls in flight (the staging slots), 2
warm-up and 5 timed rounds of 3 calls, 64-byte and 1,024-byte messages.  Call rate =
signatures / host time of a round (every call ends in a stream synchronise); kernel times
are the HIP events of the last call (fts_ecdsa_sign_last_timings, fts_nym_sign_last_timings),
min and median over the timed rounds.  Every message is distinct, so every nonce and every
table row gathered is (repeated scalars would gather the same rows from cache);
keys cycle through 64 (ECDSA) / 16 (nym) distinct ones, which the signing kernels cannot
tell from 65,536.  What was timed is then verified on the device (every verdict FTS_OK),
which also gives k_ecdsa_verify / k_nym_verify / k_nym_verify_fbn on the same items (the nym labels
name k_nym_sign<BnCurve> / k_nym_sign<FbnCurve>, the BN254 k_nym_verify and k_nym_verify<FbnCurve>).

CPU column: `openssl speed ecdsap256` sign/s of one core times 16 (the cores a caller of
this library has), if an openssl binary exists; otherwise none is recorded.

Each configuration is a child process (`--mode ...`) that prints one JSON line; a child
that fails ends the run."""
import argparse
import ctypes as C
import json
import os
import random
import re
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fabric-token-sdk_amd"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden", "idemix_golden.json")


def _med(x):
    return sorted(x)[len(x) // 2]


def _messages(n, mlen, seed):
    buf = np.frombuffer(random.Random(seed).randbytes(n * mlen), dtype=np.uint8)
    return buf, np.arange(n, dtype=np.uint64) * np.uint64(mlen), np.full(n, mlen, dtype=np.uint64)


def _rounds(a, one_call, kernel_ms):
    """a.inflight concurrent calls per round -> (signatures/s per timed round, kernel ms per timed round)"""
    rates, kms = [], []
    with ThreadPoolExecutor(a.inflight) as ex:
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            list(ex.map(one_call, range(a.inflight)))
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                rates.append(a.inflight * a.n / dt)
                kms.append(kernel_ms())
    return rates, kms


def _report(a, what, rates, kms, extra):
    d = {"what": what, "n_per_call": a.n, "inflight": a.inflight, "msg_len": a.msg_len,
         "signatures_per_s": [round(r, 1) for r in rates], "signatures_per_s_median": round(_med(rates), 1),
         "kernel_ms": {k: {"min": round(min(v[k] for v in kms), 4), "median": round(_med([v[k] for v in kms]), 4)}
                       for k in kms[0]}}
    k = [x for x in kms[0] if "sign" in x][0]
    d["kernel_signatures_per_s"] = round(a.n / (d["kernel_ms"][k]["min"] * 1e-3), 1)
    d.update(extra)
    print(json.dumps(d))


def mode_ecdsa(a):
    from fts_gpu import _lib as L, ecdsa as G
    from oracle import ecdsa_p256 as E
    rng = random.Random(256)
    keys = [rng.randrange(1, E.N) for _ in range(64)]
    pubs = [E.mul(d, E.G) for d in keys]
    n = a.n
    mbuf, moff, mlen = _messages(n, a.msg_len, 1)
    dbuf = np.frombuffer(b"".join(keys[i % 64].to_bytes(32, "big") for i in range(n)), dtype=np.uint8)
    pkbuf = b"".join(pubs[i % 64][0].to_bytes(32, "big") + pubs[i % 64][1].to_bytes(32, "big") for i in range(n))
    items = np.zeros(n, dtype=[("msg", "u8"), ("msg_len", "u8"), ("d32", "u8")])
    items["msg"], items["msg_len"] = mbuf.ctypes.data + moff, mlen
    items["d32"] = dbuf.ctypes.data + 32 * np.arange(n, dtype=np.uint64)
    mode = L.FTS_NONCE_HEDGED if a.mode == "ecdsa_hedged" else L.FTS_NONCE_RFC6979
    out = [(np.zeros(n * 72, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32))
           for _ in range(a.inflight)]

    def call(j):
        sig, ln, st = out[j]
        L.check("fts_ecdsa_sign_batch",
                L.lib.fts_ecdsa_sign_batch(0, n, items.ctypes.data_as(C.POINTER(L.EcdsaSignItem)), mode, 1000 + j * n,
                                           sig.ctypes.data, ln.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           st.ctypes.data_as(C.POINTER(C.c_int32))))
    rates, kms = _rounds(a, call, G.sign_last_timings)
    sig, ln, st = out[0]
    assert not st.any()
    vk = []
    for _ in range(4):  # the first one warms the verify kernel up
        v = G.verify_packed(mbuf, moff, mlen, sig, 72 * np.arange(n, dtype=np.uint64), ln, pkbuf)
        assert not v.any(), "a device signature failed the device verifier"
        vk.append(G.last_timings()["k_ecdsa_verify"])
    _report(a, "fts_ecdsa_sign_batch " + a.mode, rates, kms,
            {"k_ecdsa_verify_ms_min": round(min(vk[1:]), 4),
             "sign_over_verify_kernel": round(min(v["k_ecdsa_sign"] for v in kms) / min(vk[1:]), 4)})


def mode_nym(a):
    from fts_gpu import _lib as L, idemix as I
    from oracle import idemix as O
    cid = 1 if a.mode == "nym_bn254" else 0
    Cv = O.CURVES[cid]
    with open(GOLD) as f:
        raw = bytes.fromhex(json.load(f)["bn254" if cid else "fp256bn"]["ipk"])
    ipk = O.parse_ipk(raw, Cv)
    dev = I.IssuerKey(raw, device=0, curve=cid)
    rng = random.Random(136 + cid)
    ids = [(rng.randrange(Cv.r), rng.randrange(Cv.r)) for _ in range(16)]
    nyms = [O.nym_bytes(ipk, O.make_nym(ipk, s, r)) for s, r in ids]
    n, nl = a.n, dev.nym_len
    mbuf, moff, mlen = _messages(n, a.msg_len, 2)
    skbuf = np.frombuffer(b"".join(ids[i % 16][0].to_bytes(32, "big") for i in range(n)), dtype=np.uint8)
    rnbuf = np.frombuffer(b"".join(ids[i % 16][1].to_bytes(32, "big") for i in range(n)), dtype=np.uint8)
    nybuf = np.frombuffer(b"".join(nyms[i % 16] for i in range(n)), dtype=np.uint8)
    idx = np.arange(n, dtype=np.uint64)
    items = np.zeros(n, dtype=[("sk32", "u8"), ("rnym32", "u8"), ("nym", "u8"), ("nym_len", "u8"), ("msg", "u8"),
                               ("msg_len", "u8")])
    items["sk32"], items["rnym32"] = skbuf.ctypes.data + 32 * idx, rnbuf.ctypes.data + 32 * idx
    items["nym"], items["nym_len"] = nybuf.ctypes.data + nl * idx, nl
    items["msg"], items["msg_len"] = mbuf.ctypes.data + moff, mlen
    out = [(np.zeros(n * 136, dtype=np.uint8), np.zeros(n, dtype=np.int32)) for _ in range(a.inflight)]

    def call(j):
        sig, st = out[j]
        L.check("fts_nym_sign_batch",
                L.lib.fts_nym_sign_batch(dev.h, n, items.ctypes.data_as(C.POINTER(L.NymSignItem)), 1000 + j * n,
                                         sig.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_int32))))
    kname = "k_nym_sign" if cid else "k_nym_sign_fbn"
    rates, kms = _rounds(a, call, lambda: {kname: dev.last_sign_kernel_ms()})
    sig, st = out[0]
    assert not st.any()
    vk = []
    for _ in range(4):
        v = dev.verify_packed(nybuf, sig, 136 * idx, np.full(n, 136, dtype=np.uint64), mbuf, moff, mlen)
        assert not v.any(), "a device signature failed the device verifier"
        vk.append(dev.last_kernel_ms())
    vname = "k_nym_verify" if cid else "k_nym_verify_fbn"
    _report(a, "fts_nym_sign_batch " + a.mode, rates, kms,
            {vname + "_ms_min": round(min(vk[1:]), 4),
             "sign_over_verify_kernel": round(min(v[kname] for v in kms) / min(vk[1:]), 4)})
    dev.close()


def cpu_column():
    exe = shutil.which("openssl")
    if not exe:
        return {"available": False, "note": "no openssl binary on the GPU machine: no CPU column"}
    out = subprocess.run([exe, "speed", "-seconds", "3", "ecdsap256"], capture_output=True, text=True, timeout=120)
    m = re.search(r"256 bits ecdsa \(nistp256\)\s+\S+\s+\S+\s+([0-9.]+)\s+([0-9.]+)", out.stdout)
    if not m:
        return {"available": False, "note": "openssl speed output not understood", "tail": out.stdout[-300:]}
    return {"available": True, "openssl_sign_per_s_one_core": float(m.group(1)),
            "openssl_verify_per_s_one_core": float(m.group(2)), "cores_assumed": 16,
            "cpu_sign_per_s": round(16 * float(m.group(1)), 1),
            "version": subprocess.run([exe, "version"], capture_output=True, text=True).stdout.strip()}


def child(mode, extra):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, *extra], capture_output=True,
                         text=True, timeout=600)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("sign_bench: child %s failed (%d); nothing more is started" % (mode, out.returncode))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    print(mode, " ".join(extra), line, flush=True)
    return json.loads(line)


MODES = ["ecdsa_rfc6979", "ecdsa_hedged", "nym_bn254", "nym_fp256bn"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all", choices=["all"] + MODES)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--msg-len", type=int, default=64)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sign.json"))
    a = ap.parse_args()
    if a.mode != "all":
        return (mode_ecdsa if a.mode.startswith("ecdsa") else mode_nym)(a)
    fwd = ["--n", str(a.n), "--inflight", str(a.inflight), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    res = {"tool": "tools/sign_bench.py", "runs": {}}
    for ml in (64, 1024):
        for m in MODES:
            res["runs"]["%s_msg%d" % (m, ml)] = child(m, fwd + ["--msg-len", str(ml)])
    res["cpu"] = cpu_column()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
