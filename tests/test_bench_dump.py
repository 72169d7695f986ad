"""bench.py --dump-outputs: the file layout, the number format and the fixed sample (host only)."""
import os

import numpy as np
import pytest
import torch

import bench


class _Chain:
    def __init__(self, **arrays):
        self.arrays = arrays

    def last_outputs(self):
        return {k: torch.from_numpy(v) for k, v in self.arrays.items()}


@pytest.fixture
def no_gpu_sync(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)


def test_small_output_is_written_whole(tmp_path, no_gpu_sync):
    a = np.arange(1000, dtype=np.float32)
    bench.dump_outputs(_Chain(am=a), str(tmp_path / "d"), 0, 1)
    got = np.load(tmp_path / "d" / "am.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a)


def test_large_output_is_a_fixed_sample(tmp_path, no_gpu_sync):
    n = bench.DUMP_MAX_ELEMS + 12345
    a = np.arange(n, dtype=np.float32)  # element = its own index (exact below 2^24)
    bench.dump_outputs(_Chain(am=a), str(tmp_path / "d1"), 0, 1)
    bench.dump_outputs(_Chain(am=a[::-1].copy()), str(tmp_path / "d2"), 0, 1)
    s1, s2 = np.load(tmp_path / "d1" / "am.npy"), np.load(tmp_path / "d2" / "am.npy")
    assert s1.dtype == np.float32 and s1.size == bench.DUMP_MAX_ELEMS
    assert np.all(np.diff(s1) > 0)                 # distinct positions, in order
    assert np.array_equal(s2, (n - 1) - s1)        # the same positions whatever the array holds
    assert s1.nbytes <= 64 << 20


def test_ranks_write_their_own_files_within_the_budget(tmp_path, no_gpu_sync):
    world = 4
    a = np.zeros(bench.DUMP_MAX_ELEMS, dtype=np.float32)
    for r in range(world):
        bench.dump_outputs(_Chain(audio=a), str(tmp_path), r, world)
    files = sorted(os.listdir(tmp_path))
    assert files == [f"audio_rank{r}.npy" for r in range(world)]
    assert sum(np.load(tmp_path / f).size for f in files) == bench.DUMP_MAX_ELEMS
