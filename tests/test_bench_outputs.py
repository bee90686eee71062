"""bench.py --dump-outputs: what is written, its dtype, and that the sample
taken from a long output is the same from run to run (CPU tensors; the GPU
round itself is covered by the -m gpu suite)."""
import argparse

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def _args(path):
    return argparse.Namespace(dump_outputs=str(path))


def test_dump_whole_output_f32(tmp_path):
    out = torch.linspace(-1, 1, 1001, dtype=torch.float32)
    bench._dump_outputs(_args(tmp_path / "d"), 0, out)
    got = np.load(tmp_path / "d" / "weights.npy")
    assert got.dtype == np.float32
    assert np.array_equal(got, out.numpy())


@pytest.mark.parametrize("dtype", [torch.float64, torch.int64, torch.int32])
def test_dump_other_dtypes_as_f64(tmp_path, dtype):
    out = torch.arange(-5, 6).to(dtype)
    bench._dump_outputs(_args(tmp_path), 0, out)
    got = np.load(tmp_path / "weights.npy")
    assert got.dtype == np.float64
    assert np.array_equal(got, out.numpy().astype(np.float64))


def test_dump_sample_is_fixed_and_capped(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 257)
    out = torch.arange(10_007, dtype=torch.float32)
    bench._dump_outputs(_args(tmp_path / "a"), 0, out)
    bench._dump_outputs(_args(tmp_path / "b"), 0, out)
    a = np.load(tmp_path / "a" / "weights.npy")
    b = np.load(tmp_path / "b" / "weights.npy")
    assert a.shape == (257,) and a.dtype == np.float32
    assert np.array_equal(a, b)
    # values are their own indices here: sorted, in range, spread over the output
    assert (np.diff(a) >= 0).all() and a[0] >= 0 and a[-1] < 10_007
    assert a[0] < 1000 and a[-1] > 9000


def test_dump_only_when_asked_and_on_rank0(tmp_path):
    out = torch.zeros(4)
    bench._dump_outputs(argparse.Namespace(dump_outputs=None), 0, out)
    bench._dump_outputs(_args(tmp_path / "r1"), 1, out)
    assert not (tmp_path / "r1").exists()


def test_default_size_cap_fits_64mb():
    assert bench.DUMP_MAX_ELEMS * 8 <= 64_000_000
