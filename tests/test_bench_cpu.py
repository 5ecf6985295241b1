"""CPU: bench.py's --dump-outputs writer (float arrays, shapes kept, the size cap
with its fixed sample) and the --full / --dump-outputs options."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    # bench.py raises GPU_MAX_HW_QUEUES for its own process on import: keep that out of this session
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    monkeypatch.syspath_prepend(ROOT)
    import bench as b
    return b


def test_dump_outputs_float_arrays_keep_shape_and_values(bench, tmp_path):
    st = np.array([[0, 3, 0, 7, 0], [0, 0, 0, 0, 12]], dtype=np.int32)
    args = argparse.Namespace(dump_outputs=str(tmp_path / "d"))
    bench._dump_outputs(args, 0, {"status": st, "blob": b"\x00\x01\xff", "f64": np.array([1.5, 2.0 ** 40 + 1])})
    got = np.load(tmp_path / "d" / "status.npy")
    assert got.dtype == np.float32 and got.shape == st.shape and (got == st).all()
    blob = np.load(tmp_path / "d" / "blob.npy")
    assert blob.dtype == np.float32 and blob.tolist() == [0.0, 1.0, 255.0]
    f64 = np.load(tmp_path / "d" / "f64.npy")
    assert f64.dtype == np.float64 and f64.tolist() == [1.5, 2.0 ** 40 + 1]


def test_dump_outputs_cap_takes_the_same_sample_every_time(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    a = np.arange(10000, dtype=np.int32)
    outs = []
    for d in ("a", "b"):
        args = argparse.Namespace(dump_outputs=str(tmp_path / d))
        bench._dump_outputs(args, 0, {"x": a, "y": a[:16]})
        x, y = np.load(tmp_path / d / "x.npy"), np.load(tmp_path / d / "y.npy")
        assert x.nbytes + y.nbytes <= 4096 and x.size == 512 and (y == a[:16]).all()
        assert (np.diff(x) > 0).all() and set(x.astype(np.int64)) <= set(range(10000))
        outs.append(x)
    assert (outs[0] == outs[1]).all()


def test_dump_outputs_only_rank0_and_only_when_asked(bench, tmp_path):
    bench._dump_outputs(argparse.Namespace(dump_outputs=str(tmp_path / "r1")), 1, {"x": np.zeros(3)})
    bench._dump_outputs(argparse.Namespace(dump_outputs=None), 0, {"x": np.zeros(3)})
    assert not (tmp_path / "r1").exists()


def test_options_are_listed():
    """the command line itself (no GPU work: --help exits before any setup)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         check=True).stdout
    assert "--full" in out and "--dump-outputs DIR" in out
