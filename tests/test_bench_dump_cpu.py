"""bench.py --dump-outputs / --full on the host: the plain run's switches, and the writer of the
last step's outputs (float .npy files inside the byte budget, a fixed seeded sample for an array
past its share, the same from run to run)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_switches():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_whole_arrays(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"images": rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8), "body_bytes": np.array([5, 7]),
              "metrics": rng.standard_normal((2, 7)).astype(np.float32), "f64": rng.standard_normal(3)}
    bench.dump_outputs(str(tmp_path), "", arrays)
    assert sorted(os.listdir(tmp_path)) == ["body_bytes.npy", "f64.npy", "images.npy", "metrics.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == (np.float64 if a.dtype == np.float64 else np.float32)
        assert got.shape == a.shape and np.array_equal(got, a)  # u8 and small ints are exact in float32


def test_dump_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = np.arange(100_003, dtype=np.float32).reshape(-1, 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "_rank1", {"images": big, "metrics": np.ones((2, 7), np.float32)})
        assert _dir_bytes(tmp_path / d) <= 4096 + 3 * 128  # payload inside the budget, plus the .npy headers
    idx = np.load(tmp_path / "a" / "images_index_rank1.npy")
    val = np.load(tmp_path / "a" / "images_rank1.npy")
    assert idx.dtype == np.float64 and val.dtype == np.float32 and idx.shape == val.shape and idx.size > 100
    assert np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < big.size
    assert np.array_equal(val, big.reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "images_index_rank1.npy"))  # the same sample every run
    assert np.array_equal(np.load(tmp_path / "a" / "metrics_rank1.npy"), np.ones((2, 7), np.float32))
