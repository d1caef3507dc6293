"""bench.py --dump-outputs on CPU: what a step returned lands as <name>.npy in float32 / float64,
integer tensors exactly, None entries dropped; over the byte budget every array keeps a fixed,
seeded sample, identical from run to run."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    return {"audio": torch.rand(2, 1, 100, generator=g),
            "codes": torch.randint(0, 1024, (2, 8, 7), generator=g),
            "vq/commitment_loss": torch.tensor(0.25, dtype=torch.float64),
            "half": torch.rand(3, 5, generator=g).to(torch.bfloat16),
            "mask_imp": None,
            "levels": [{"bpf": 3.5, "mask": torch.ones(2, 3, dtype=torch.bool)}]}


def test_dump_names_dtypes_values(tmp_path):
    out = _outputs()
    bench.dump_outputs(out, str(tmp_path / "d"))
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["audio", "codes", "half", "levels_0_bpf", "levels_0_mask",
                           "vq_commitment_loss"]
    assert got["audio"].dtype == np.float32 and got["audio"].shape == (2, 1, 100)
    np.testing.assert_array_equal(got["audio"], out["audio"].numpy())
    assert got["codes"].dtype == np.float64
    np.testing.assert_array_equal(got["codes"], out["codes"].numpy())
    assert got["vq_commitment_loss"].dtype == np.float64 and got["vq_commitment_loss"] == 0.25
    assert got["half"].dtype == np.float32
    np.testing.assert_array_equal(got["half"], out["half"].float().numpy())
    assert got["levels_0_bpf"] == 3.5
    assert got["levels_0_mask"].dtype == np.float64 and got["levels_0_mask"].sum() == 6


def test_dump_budget_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    out = {"a": torch.arange(3000, dtype=torch.float32).reshape(30, 100),
           "b": torch.arange(500), "s": torch.tensor(1.0)}
    bench.dump_outputs(out, str(tmp_path / "x"))
    bench.dump_outputs(out, str(tmp_path / "y"), suffix=".rank1")
    total = 0
    for name in ("a", "b", "s"):
        x = np.load(tmp_path / "x" / f"{name}.npy")
        y = np.load(tmp_path / "y" / f"{name}.rank1.npy")
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
        assert x.ndim == 1 and np.all(np.diff(x) > 0)  # a sorted subset of the flat array
    assert total <= 4000
    a = np.load(tmp_path / "x" / "a.npy")
    assert 0 < a.size < 3000 and set(a.tolist()) <= set(range(3000))
