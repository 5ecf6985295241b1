"""CPU: the prover side of the multi-device layer without a device --
fts_debug_shard_work on contexts that have no device work to count, the header as
strict C11, and the device provers' answer on a parent whose children are host-only."""
import ctypes as C
import os
import shutil
import subprocess

from conftest import ROOT

EINVAL, EDEVICE = -1, -3


def test_shard_work_needs_a_device(host_pp, pp_raw):
    import fts_gpu
    from fts_gpu import _lib as L
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    pp = host_pp(8)
    assert L.lib.fts_debug_shard_work(pp._ctx, 0, out) == EINVAL
    assert L.lib.fts_debug_shard_work(None, 0, out) == EINVAL
    assert L.lib.fts_debug_shard_work(pp._ctx, 0, None) == EINVAL
    assert tuple(out) == (7, 7, 7, 7)
    try:
        pp.shard_work()
    except L.FtsError as e:
        assert e.code == EINVAL
    else:
        raise AssertionError("shard_work on a host-only context did not raise")
    # children that are host-only: the shard index is checked, then the child answers
    multi = fts_gpu.PublicParams(pp_raw, bit_length=8, devices=[fts_gpu.FTS_DEVICE_NONE] * 2)
    for shard in (-1, 0, 1, 2):
        assert L.lib.fts_debug_shard_work(multi._ctx, shard, out) == EINVAL
    assert L.lib.fts_debug_shard_timings(multi._ctx, 2, None, None, 0) == 0
    multi.close()


def test_header_is_strict_c11(tmp_path):
    """include/fts_gpu.h with fts_debug_shard_work's int64_t out[4] parameter, as C"""
    with open(os.path.join(ROOT, "include", "fts_gpu.h")) as f:
        assert "int fts_debug_shard_work(const fts_ctx* ctx, int shard, int64_t out[4]);" in f.read()
    cc = next((p for p in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"),
                           "/opt/rocm/llvm/bin/clang") if p and os.path.exists(p)), None)
    assert cc, "no C compiler"
    src = tmp_path / "hdr.c"
    src.write_text('#include "fts_gpu.h"\n'
                   "int use(const fts_ctx* c) { int64_t w[4]; return fts_debug_shard_work(c, 0, w); }\n")
    out = subprocess.run([cc, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                          "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr


def test_device_provers_on_host_only_parent(host_pp, pp_raw):
    """a host-only context, and a multi-device parent whose children are host-only:
    FTS_API_EDEVICE from every sharded entry point, nothing written"""
    import fts_gpu as F
    from fts_gpu import _lib as L
    multi = F.PublicParams(pp_raw, bit_length=8, devices=[F.FTS_DEVICE_NONE] * 2)
    assert multi.devices == [F.FTS_DEVICE_NONE] * 2
    bf = [(5).to_bytes(32, "big"), (6).to_bytes(32, "big")]
    wit = F.WitnessBatch([(b"ABC", [3, 4], bf, [2, 5], bf)] * 3, 3)
    iss = F.WitnessBatch([(b"ABC", [], [], [2, 5], bf)] * 3, 3)
    gen = F.GenBatch([(b"ABC", [(b"tx", 0, b"alice", bytes(64), 7, bf[0])], [(7, b"bob")], b"")] * 3, 3)
    for pp in (host_pp(8), multi):
        for call in (lambda: pp.prove_range_batch_gpu([1, 2, 3], bf + bf[:1], 1),
                     lambda: pp.prove_transfers_gpu(wit, 1), lambda: pp.prove_issues_gpu(iss, 1),
                     lambda: pp.token_commit_batch_gpu([(b"ABC", 1, bf[0])] * 3),
                     lambda: pp.generate_transfers_gpu(gen, 1), lambda: pp.generate_issues_gpu(gen, 1)):
            try:
                call()
            except L.FtsError as e:
                assert e.code == EDEVICE
            else:
                raise AssertionError("a device prover ran without a device")
    multi.close()
