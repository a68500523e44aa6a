"""bench.py --dump-outputs: the writer's size budget and sampling (no GPU needed)."""
import numpy as np
import torch


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """An output over the 64 MB budget is cut to the same seeded sample every time."""
    import bench
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4096)
    x = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    small = torch.arange(6, dtype=torch.float64)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'x': x, 'small': small})
    a, b = (np.load(tmp_path / d / 'x.npy') for d in ('a', 'b'))
    assert a.dtype == np.float32 and a.nbytes <= 2048 and a.size == 512
    assert np.array_equal(a, b) and np.all(np.diff(a) >= 0) and a.max() < 5000
    s = np.load(tmp_path / 'a' / 'small.npy')
    assert s.dtype == np.float64 and np.array_equal(s, np.arange(6.0))
