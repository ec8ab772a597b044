"""CPU: bench.py --dump-outputs. dump_outputs writes the outputs of one pipeline slot as
float64 .npy files: every row of a small batch, a fixed seeded sample of DUMP_ROWS rows of
a larger one (the same rows on every run), within 64 MB in all."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Engine:
    def stats(self):
        return {"n_distinct": 5, "n_clusters": 3, "overflow": 0, "error": 0}


class _Slot:
    def __init__(self, count):
        from rogtk_amd import device as D

        self.eng = _Engine()
        self.scores = D.alloc_scores(count, "cpu")
        for i, t in enumerate(self.scores.values()):  # field i of row r holds r + i
            t.copy_((torch.arange(t.numel()) + i).to(t.dtype))
        self.cid = (torch.arange(max(count, 4), dtype=torch.int64) * 3).to(torch.int32)
        self.within = torch.full(((count + 63) // 64,), 0x5555555555555555, dtype=torch.int64)  # even rows set


@pytest.fixture(scope="module")
def bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench as B
    finally:
        sys.argv = argv
    return B


@pytest.mark.parametrize("sampled", [False, True])
def test_dump_outputs(bench, tmp_path, monkeypatch, sampled):
    count = 1000
    if sampled:
        monkeypatch.setattr(bench, "DUMP_ROWS", 300)
    slot = _Slot(count)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), slot, count, 0, 1)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == set(slot.scores) | {"rows", "cluster_id", "hamming_within", "cluster_stats"}
    assert all(a.dtype == np.float64 for a in got.values())
    for name, a in got.items():  # the same rows and values on every run
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))
    rows = got["rows"].astype(np.int64)
    assert len(rows) == (300 if sampled else count) and np.all(np.diff(rows) > 0) and rows[-1] < count
    for i, f in enumerate(slot.scores):
        assert np.array_equal(got[f], rows + i), f
    assert np.array_equal(got["cluster_id"], rows * 3)
    assert np.array_equal(got["hamming_within"], rows % 2 == 0)
    assert got["cluster_stats"].tolist() == [5, 3, 0]


def test_dump_budget(bench):
    # 7 H1 fields + ids + within bits + the row indices, float64, of DUMP_ROWS rows
    assert 10 * 8 * bench.DUMP_ROWS <= 64 * 1000 * 1000
