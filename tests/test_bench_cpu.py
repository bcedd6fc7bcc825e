"""bench.py's --dump-outputs writer (no device work): float32 files, the 64 MB cap and its seeded sample."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_float32_arrays_whole_under_the_cap(tmp_path):
    images = np.random.default_rng(1).integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"images": images, "actions": np.linspace(-1, 1, 32).reshape(2, 2, 8)})
    got = np.load(tmp_path / "images.npy")
    assert got.dtype == np.float32 and got.shape == images.shape and (got == images).all()
    assert np.load(tmp_path / "actions.npy").dtype == np.float32
    assert sorted(os.listdir(tmp_path)) == ["actions.npy", "images.npy"]


def test_dump_outputs_samples_the_same_elements_over_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 16)
    big, small = np.arange(1 << 16, dtype=np.float64), np.ones(10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))  # minus the .npy headers
    assert total <= 1 << 16
    idx, vals = np.load(tmp_path / "a" / "big_index.npy"), np.load(tmp_path / "a" / "big.npy")
    assert vals.dtype == np.float32 and (vals == big[idx]).all() and len(np.unique(idx)) == len(idx)
    assert (idx == np.load(tmp_path / "b" / "big_index.npy")).all()
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
