"""CPU-only checks of `bench.py --dump-outputs`: the files, their dtype, the size budget and the fixed sample of a solution
larger than its share of the budget.  (The dump of a real run is checked on the GPU in test_gpu_parity.py.)"""

import types

import numpy as np
import torch

import bench


def _results(sizes, seed):
    rng = np.random.default_rng(seed)
    return [types.SimpleNamespace(x=torch.from_numpy(rng.standard_normal(n))) for n in sizes]


def test_dump_writes_records_and_whole_solutions(tmp_path):
    table = np.array([[187.0, 0.0, 9.7e-9, 0.004], [190.0, 0.0, 8.1e-9, 0.005]])
    res = _results([1000, 1000], seed=1)
    bench.dump_outputs(tmp_path, table, [0, 1], res, 2, torch)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["records.npy", "x_system0.npy", "x_system1.npy"]
    rec = np.load(tmp_path / "records.npy")
    assert rec.dtype == np.float64 and np.array_equal(rec, table[:, :3])          # the wall time is not an output
    for i, r in enumerate(res):
        x = np.load(tmp_path / f"x_system{i}.npy")
        assert x.dtype == np.float64 and np.array_equal(x, r.x.numpy())


def test_dump_samples_what_exceeds_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 1024)
    res = _results([50_000, 50_000, 100], seed=2)
    # this rank holds systems 4, 7, 10 of a batch of 12; no records (not rank 0)
    bench.dump_outputs(tmp_path / "a", None, [4, 7, 10], res, 12, torch)
    bench.dump_outputs(tmp_path / "b", None, [4, 7, 10], res, 12, torch)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["x_system10.npy", "x_system4.npy", "x_system7.npy"]
    total = 0
    for name in files:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b)                       # the same sample every time
        total += (tmp_path / "a" / name).stat().st_size
    assert total * 12 / 3 <= 64 * 1024                                                 # every system's share fits the budget
    share = np.load(tmp_path / "a" / "x_system4.npy").size
    assert 0 < share < 50_000
    idx = np.sort(np.random.default_rng(0).choice(50_000, share, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "x_system4.npy"), res[0].x.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "x_system10.npy"), res[2].x.numpy())    # small enough: whole
