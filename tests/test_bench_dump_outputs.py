"""bench.py --dump-outputs writes the frame of the timed path's last step (no GPU needed for the writer): a frame within
the limit as it is, float32; a larger one as a fixed, seeded sample of its pixels with their indices, within the limit."""
import os

import numpy as np

from test_bench_live_counters import load_bench


def test_a_frame_within_the_limit_is_written_whole(tmp_path):
    bench = load_bench()
    img = np.random.RandomState(3).uniform(0, 2, (9, 16, 4)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "out"), img)
    assert sorted(os.listdir(tmp_path / "out")) == ["image.npy"]
    got = np.load(tmp_path / "out" / "image.npy")
    assert got.dtype == np.float32 and got.shape == img.shape
    assert np.array_equal(got.view(np.uint32), img.view(np.uint32))


def test_a_larger_frame_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    bench = load_bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    img = np.random.RandomState(4).uniform(0, 2, (90, 160, 4)).astype(np.float32)   # 225 KB
    written = []
    for run in ("a", "b"):
        d = tmp_path / run
        bench.dump_outputs(str(d), img)
        assert sorted(os.listdir(d)) == ["image.npy", "pixel_index.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 10
        written.append((np.load(d / "image.npy"), np.load(d / "pixel_index.npy")))
    (sample, index), (sample_b, index_b) = written
    assert sample.dtype == np.float32 and index.dtype == np.float64
    assert np.array_equal(index, index_b) and np.array_equal(sample, sample_b)   # the same pixels every run
    idx = index.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 90 * 160 and len(idx) > 1000
    assert np.array_equal(sample, img.reshape(-1, 4)[idx])
