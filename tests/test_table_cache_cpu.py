"""CPU: the table cache (csrc/host/table_cache.hpp) driven over host memory by a
plain program built with the host address / undefined-behaviour sanitizers (a
report aborts it) -- no HIP, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT


def test_table_cache_check():
    """lib/table_cache_check (csrc/tools/table_cache_check.cpp): 16 threads on one key
    build once and all read the built table; a failed first build wakes the waiters
    and exactly one of them builds again; builder-first and builder-last release free
    the table once and return the books to zero; private entries stay out of the
    books; two keys build concurrently"""
    exe = os.path.join(ROOT, "fabric-token-sdk_amd", "lib", "table_cache_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "table_cache_check: ok" in out.stdout


def test_header_declares_the_table_calls():
    """include/fts_gpu.h carries both calls and the library exports them (the struct of
    the cache's books shares its name with the call, so it is no typedef)"""
    from fts_gpu import _lib as L
    with open(os.path.join(ROOT, "include", "fts_gpu.h")) as f:
        src = f.read()
    assert "int fts_ctx_table_info(const fts_ctx* ctx, int shard, fts_table_info* out);" in src
    assert "int fts_table_cache_stats(int device, struct fts_table_cache_stats* out);" in src
    assert hasattr(L.lib, "fts_ctx_table_info") and hasattr(L.lib, "fts_table_cache_stats")
    # no device needed: an unused device has empty books; a host-only context has no tables
    import fts_gpu
    assert tuple(fts_gpu.table_cache_stats(63)) == (0, 0, 0, 0)
