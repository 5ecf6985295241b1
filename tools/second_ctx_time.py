#!/usr/bin/env python3
"""Wall time of creating a second default context beside a first on one device
(DESIGN.md §4.1): with shared tables the second creation builds nothing.

    python tools/second_ctx_time.py [--bits 64] [--device 0]
    FTS_LIB=<libfts_gpu.so of another revision> python tools/second_ctx_time.py

Prints one JSON line: creation seconds, window widths and table bytes of both
contexts, the device's free memory after each, and (where the library has the call)
the second context's table_info."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fabric-token-sdk_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch
    import fts_gpu
    with open(os.path.join(ROOT, "tests", "golden", "zkatdlog_pp.json"), "rb") as f:
        raw = f.read()
    torch.cuda.init()
    torch.cuda.mem_get_info(args.device)  # the device's runtime is up before the clock starts
    out = {"lib": fts_gpu._lib.LIB_PATH, "bits": args.bits}
    ctxs = []
    for name in ("first", "second"):
        t0 = time.perf_counter()
        pp = fts_gpu.PublicParams(raw, bit_length=args.bits, device=args.device)
        out[name] = {"create_s": round(time.perf_counter() - t0, 3), "wide_bits": pp.wide_bits,
                     "table_bytes": pp.table_bytes, "free_bytes_after": torch.cuda.mem_get_info(args.device)[0]}
        if hasattr(fts_gpu._lib.lib, "fts_ctx_table_info") and hasattr(pp, "table_info"):
            out[name]["table_info"] = pp.table_info()._asdict()
        ctxs.append(pp)
    for pp in ctxs:
        pp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
