#!/usr/bin/env python3
"""Stage times of fts_idemix_cred_verify_batch beside fts_idemix_identity_verify_batch, same
process, same handle, same n, the two calls alternating:
    python tools/cred_verify_bench.py [--items 16384] [--rounds 7] [--out profiles/cred_verify.json]
BN254: 64 credentials issued with the oracle under bn254_tokengen, tiled, all honest; the
identities are generated on the device from the first of them.  FP256BN: the two reference
credentials under fp256bn_validator, tiled; identities from the first.  Tiled inputs repeat
scalars, so the fixed-base table gathers are cache-friendlier than real traffic."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fabric-token-sdk_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def measure(issuer, creds, n, rounds):
    from fts_gpu import idemix as I
    import cred_common as K
    V = I.IdentityVerifier(K.raw(issuer, "IssuerPublicKey"), device=0, curve=K.ISSUERS[issuer][0])
    try:
        dev = I.Credential(V, creds[0][0], creds[0][1])
        try:
            g = dev.generate(n, seed=11)
        finally:
            dev.close()
        assert not g.status.any()
        prep = V.prepare(g.ids)
        cl, sl = [creds[i % len(creds)][0] for i in range(n)], [creds[i % len(creds)][1] for i in range(n)]
        cred_ms, id_ms = [], []
        for r in range(rounds + 1):  # the first round warms both paths up
            assert not V.verify_prepared(prep).any()
            a = V.last_kernel_ms()
            assert not V.verify_credentials(cl, sl).any()
            b = V.last_cred_kernel_ms()
            assert V.last_cred_stats() == ((n + 255) // 256, 0) and V.last_pairing_stats() == ((n + 255) // 256, 0)
            if r:
                id_ms.append(a), cred_ms.append(b)
        med = lambda xs, k: round(statistics.median(x[k] for x in xs), 4)  # noqa: E731
        return {"items": n, "distinct_credentials": len(creds), "rounds": rounds,
                "cred_ms": [[round(x, 4) for x in t] for t in cred_ms],
                "identity_ms": [[round(x, 4) for x in t] for t in id_ms],
                "cred_prep_ms_median": med(cred_ms, 0), "cred_pairing_ms_median": med(cred_ms, 1),
                "identity_tvals_ms_median": med(id_ms, 0), "identity_pairing_ms_median": med(id_ms, 1),
                "prep_over_identity_stage0": round(med(cred_ms, 0) / med(id_ms, 0), 3),
                "pairing_over_identity_stage1": round(med(cred_ms, 1) / med(id_ms, 1), 3)}
    finally:
        V.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cred_verify.json"))
    a = ap.parse_args()
    import cred_common as K
    rng = random.Random(1)
    sk = lambda k: k["sk"].to_bytes(32, "big")  # noqa: E731
    bn = [K.issue_bn254(rng) for _ in range(64)]
    fb = [K.signer("fp256bn_validator"), K.signer("fp256bn_validator", "SignerConfig2")]
    doc = {"tool": "tools/cred_verify_bench.py",
           "inputs": "tiled credentials, all honest (asserted); tiling repeats scalars, so the fixed-base table "
                     "gathers are cache-friendlier than real traffic",
           "stages": "cred: [0] k_cred_decode + k_cred_var + k_cred_join, [1] pairing stage; identity: [0] k_idv_decode "
                     "+ k_idv_var + k_idv_tvals, [1] pairing stage; HIP-event ms, medians over the rounds, the two "
                     "calls alternating on one handle in one process",
           "bn254": measure("bn254_tokengen", [(K.cred_proto(k), sk(k)) for k in bn], a.items, a.rounds),
           "fp256bn": measure("fp256bn_validator", [(K.cred_proto(k), sk(k)) for k in fb], a.items, a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: {m: v for m, v in doc[k].items() if m.endswith("median") or "over" in m} for k in ("bn254", "fp256bn")}))


if __name__ == "__main__":
    main()
