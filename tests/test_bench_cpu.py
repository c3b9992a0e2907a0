"""bench.py --dump-outputs on a stand-in engine: file names, float32, the size cap, and the same sample positions on every run."""
import os
import types

import numpy as np
import torch

import bench


def _engine(n):
    # value == position, so a sample shows which positions it took
    return types.SimpleNamespace(flat=torch.arange(n, dtype=torch.float32), grad=-torch.arange(n, dtype=torch.float32))


def test_dump_outputs_writes_small_buffers_whole(tmp_path):
    bench.dump_outputs(str(tmp_path), torch.tensor(2.5), _engine(1000))
    assert sorted(os.listdir(tmp_path)) == ["grad.npy", "loss.npy", "trainable.npy"]
    d = {k: np.load(tmp_path / (k + ".npy")) for k in ("loss", "grad", "trainable")}
    assert all(v.dtype == np.float32 for v in d.values())
    assert d["loss"].tolist() == [2.5]
    assert np.array_equal(d["trainable"], np.arange(1000, dtype=np.float32)) and np.array_equal(d["grad"], -d["trainable"])


def test_dump_outputs_samples_large_buffers_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), torch.tensor(1.0), _engine(1000))
    a, b = (np.load(tmp_path / run / "trainable.npy") for run in ("a", "b"))
    assert a.shape == (64,) and np.array_equal(a, b)
    assert (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 1000      # distinct positions, in order, in range
    assert np.array_equal(np.load(tmp_path / "a" / "grad.npy"), -a)    # both buffers sampled at the same positions


def test_dump_outputs_stay_under_64_mb():
    assert 2 * bench.DUMP_SAMPLE * 4 + 4 <= 64 * 2 ** 20
