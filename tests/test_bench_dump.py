"""bench.py --dump-outputs: every numeric leaf of the step's outputs lands as <name>.npy in float32 / float64, the files stay
within the byte budget, and the sample of an over-budget array is the same from run to run."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    return {"loss": torch.tensor(1.5, requires_grad=True) * 2,
            "outputs": {"big": torch.randn(3_000_000, generator=g), "ids": torch.arange(10, dtype=torch.int64),
                        "mask": torch.tensor([True, False]), "half": torch.ones(4, 2, dtype=torch.bfloat16),
                        "list": [torch.zeros(3, dtype=torch.float64), 7], "ref_iou_rate_0.25": 0.5, "note": "text", "none": None}}


def test_dump_writes_every_numeric_leaf_within_budget(tmp_path):
    budget = 4 << 20
    man = bench.dump_outputs(str(tmp_path), _outputs(), meta={"steps": 3}, budget=budget)
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert files == sorted(["loss.npy", "outputs.big.npy", "outputs.ids.npy", "outputs.mask.npy", "outputs.half.npy",
                            "outputs.list.0.npy", "outputs.list.1.npy", "outputs.ref_iou_rate_0.25.npy"])
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= budget
    load = lambda n: np.load(os.path.join(tmp_path, n + ".npy"))
    assert load("loss").dtype == np.float32 and float(load("loss")) == 3.0
    assert load("outputs.ids").dtype == np.float64 and np.array_equal(load("outputs.ids"), np.arange(10))
    assert load("outputs.mask").dtype == np.float64 and load("outputs.mask").tolist() == [1.0, 0.0]
    assert load("outputs.half").dtype == np.float32 and load("outputs.half").shape == (4, 2)
    assert load("outputs.list.0").dtype == np.float64 and float(load("outputs.list.1")) == 7.0
    big = load("outputs.big")
    assert big.dtype == np.float32 and 0 < big.size < 3_000_000 and man["outputs.big"]["sampled"] == big.size
    assert man["outputs.big"]["shape"] == [3_000_000] and man["outputs.ids"]["sampled"] is None
    # the sample is values of the array itself, at sorted flat indices
    full = _outputs()["outputs"]["big"].numpy()
    assert np.isin(big, full).all()
    assert json.load(open(os.path.join(tmp_path, "manifest.json")))["meta"] == {"steps": 3}


def test_dump_sample_is_the_same_in_every_run(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, _outputs(), budget=2 << 20)
    bench.dump_outputs(b, _outputs(), budget=2 << 20)
    for f in sorted(os.listdir(a)):
        if f.endswith(".npy"):
            assert np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))), f
