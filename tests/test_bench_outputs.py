"""CPU: bench.py --dump-outputs helpers -- what is kept of a step, and the 64 MB budget with its fixed row sample."""
import os

import numpy as np
import torch

import bench


def test_last_step_keeps_only_the_armed_last_step():
    keep = bench.LastStep(4)
    x = torch.zeros(2, requires_grad=True)
    x.grad = torch.ones(2)
    keep(3, "img", "radii", {"_points": x})            # not armed: an untimed step
    assert keep.taken == {}
    keep.armed = "single"
    keep(2, "img2", "radii2", {"_points": x})          # not the last step
    assert keep.taken == {}
    keep(3, "img3", "radii3", {"_points": x, "other": torch.zeros(1, requires_grad=True)})
    assert set(keep.taken) == {"single"}
    t = keep.taken["single"]
    assert t["color"] == "img3" and t["radii"] == "radii3" and set(t) == {"color", "radii", "grad_points"}


def test_write_outputs_float32_and_budget(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"color": torch.rand(3, 8, 8, generator=g), "radii": torch.arange(1000, dtype=torch.int32),
              "grad_a": torch.rand(1000, 3, generator=g), "grad_b": torch.rand(1000, 2, dtype=torch.float64, generator=g)}
    shapes = bench.write_outputs(str(tmp_path / "all"), arrays)
    assert shapes == {"color": [3, 8, 8], "radii": [1000], "grad_a": [1000, 3], "grad_b": [1000, 2]}
    r = np.load(tmp_path / "all" / "radii.npy")
    assert r.dtype == np.float32 and np.array_equal(r, np.arange(1000, dtype=np.float32))
    assert np.load(tmp_path / "all" / "grad_b.npy").dtype == np.float64

    budget = 30_000
    s1 = bench.write_outputs(str(tmp_path / "s1"), arrays, budget=budget)
    s2 = bench.write_outputs(str(tmp_path / "s2"), arrays, budget=budget)
    assert s1 == s2 and s1["color"] == [3, 8, 8] and s1["radii"][0] < 1000
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= budget
    rows = np.load(tmp_path / "s1" / "radii.npy").astype(np.int64)            # radii[i] == i: the sampled row indices
    assert (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / "s1" / "grad_a.npy"), arrays["grad_a"].numpy()[rows])
    for f in os.listdir(tmp_path / "s1"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)), f
