"""bench.py --dump-outputs: what the files hold and that they stay within their byte budget.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench
from conftest import ROOT


def _frame(h, w):
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=g)


def test_dump_writes_the_whole_frame_and_the_counts(tmp_path):
    frame = _frame(1080, 1920)  # BASELINE config 4, the default line
    bench.dump_outputs(str(tmp_path), frame, [1.0, 2.0, 3.0, 4.0])
    assert sorted(os.listdir(tmp_path)) == ["frame_rgba8.npy", "path_counts.npy"]
    img = np.load(tmp_path / "frame_rgba8.npy")
    assert img.dtype == np.float32 and img.shape == (1080, 1920, 4)
    assert np.array_equal(img, frame.numpy().astype(np.float32))
    counts = np.load(tmp_path / "path_counts.npy")
    assert counts.dtype == np.float64 and counts.tolist() == [1.0, 2.0, 3.0, 4.0]


def test_dump_of_a_large_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    frame = _frame(2160, 3840)  # BASELINE config 5: the whole frame as float32 would be 133 MB
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), frame, [0.0] * 4)
    bench.dump_outputs(str(b), frame, [0.0] * 4)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BYTES
    idx = np.load(a / "frame_pixel_index.npy")
    px = np.load(a / "frame_rgba8.npy")
    assert idx.dtype == np.float64 and px.dtype == np.float32 and px.shape == (idx.size, 4)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 2160 * 3840
    assert np.array_equal(px, frame.numpy().reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(b / "frame_pixel_index.npy"))  # the same pixels every run


def test_dump_needs_a_timed_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--dump-outputs needs at least one timed step" in r.stderr
