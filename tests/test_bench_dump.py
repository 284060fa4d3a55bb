"""bench.py --dump-outputs: the frame of the last timed step as float32 .npy files, at most 64 MB in all, the same
files for the same frame (a seeded pixel sample above the limit)."""
import os

import numpy as np

import bench


def _frame(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 4), dtype=np.uint8)


def test_whole_frame_at_1080p(tmp_path):
    f = _frame(1920, 1080, 1)
    names = bench.dump_outputs(str(tmp_path), f)
    assert names == ["frame_rgba8.npy"]
    got = np.load(os.path.join(str(tmp_path), "frame_rgba8.npy"))
    assert got.dtype == np.float32 and got.shape == (1080, 1920, 4)
    assert np.array_equal(got, f.astype(np.float32))


def test_sample_above_the_limit_is_fixed_and_bounded(tmp_path):
    f = _frame(3840, 2160, 2)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    names = bench.dump_outputs(a, f)
    assert bench.dump_outputs(b, f) == names == ["frame_rgba8.npy", "frame_rgba8_index.npy"]
    total = sum(os.path.getsize(os.path.join(a, n)) for n in names)
    assert total <= 64 * 1000 * 1000
    vals = np.load(os.path.join(a, "frame_rgba8.npy"))
    idx = np.load(os.path.join(a, "frame_rgba8_index.npy"))
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and vals.shape == (idx.size, 4)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 3840 * 2160
    assert np.array_equal(vals, f.reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    for n in names:                      # the same frame gives the same files
        assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n)))
