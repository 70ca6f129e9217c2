"""CPU tier: bench.py's --dump-outputs writer (no GPU: it takes any torch tensor).  Everything fits under the limit: the
arrays are written whole, in float64.  More than the limit: the same seeded, sorted sample of rows from every array, the
same on every call, and never more than the limit in all."""
import importlib
import os

import numpy as np
import torch


def _bench():
    return importlib.import_module("bench")


def test_dump_outputs_writes_small_arrays_whole(tmp_path):
    bench = _bench()
    core = torch.arange(60, dtype=torch.float64).reshape(5, 12)
    pred = torch.linspace(-1, 1, 21, dtype=torch.float64).reshape(7, 3)
    written = bench.dump_outputs(str(tmp_path / "out"), {"core": core, "predictions": pred})
    assert written == {"core": [5, 5], "predictions": [7, 7]}
    got = np.load(tmp_path / "out" / "core.npy")
    assert got.dtype == np.float64 and np.array_equal(got, core.numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "predictions.npy"), pred.numpy())


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    rows = 2000
    core = torch.arange(rows, dtype=torch.float64)[:, None].repeat(1, 14)        # row r holds r in every column
    inf = -torch.arange(rows, dtype=torch.float64)[:, None].repeat(1, 10)
    w1 = bench.dump_outputs(str(tmp_path / "a"), {"core": core, "inference": inf})
    w2 = bench.dump_outputs(str(tmp_path / "b"), {"core": core, "inference": inf})
    assert w1 == w2
    a_core, a_inf = np.load(tmp_path / "a" / "core.npy"), np.load(tmp_path / "a" / "inference.npy")
    assert a_core.nbytes + a_inf.nbytes <= 40_000
    assert 0 < a_core.shape[0] < rows and a_core.shape[1] == 14
    idx = a_core[:, 0]
    assert np.all(np.diff(idx) > 0)                                  # sorted, no row twice
    assert np.array_equal(a_core, core.numpy()[idx.astype(np.int64)])
    assert np.array_equal(a_inf[:, 0], -idx)                         # the same rows of every array
    assert np.array_equal(np.load(tmp_path / "b" / "core.npy"), a_core)
    for name in ("core.npy", "inference.npy"):
        assert os.path.getsize(tmp_path / "a" / name) < 40_000
