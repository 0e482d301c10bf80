"""CPU: bench.py's --dump-outputs writer (float32 / float64 files, 64 MB budget, seeded row samples)."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("mtgv_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _step(F=32, K=8):
    g = torch.Generator().manual_seed(0)
    return {
        "ids": torch.randint(0, 100_000, (F, K, 1), generator=g),
        "scores": torch.rand((F, K, 1), generator=g),
        "n_det": torch.randint(0, 300, (F,), generator=g, dtype=torch.int32),
        "boxes": torch.rand((F, K, 4), generator=g),
        "crops": torch.randint(0, 256, (F * K, 192, 128, 3), generator=g, dtype=torch.uint8),
        "z": torch.randn((F * K, 768), generator=g),
        "det": {"n_det": torch.zeros((F,), dtype=torch.int32), "mask_logits": torch.randn((F, K, 160, 160), generator=g), "none": None},
    }


def test_dump_outputs_budget_and_dtypes(tmp_path):
    bench = _bench()
    step = _step()
    written = bench.dump_outputs(step, str(tmp_path))
    files = sorted(os.listdir(tmp_path))
    assert {"ids.npy", "scores.npy", "n_det.npy", "boxes.npy", "crops.npy", "z.npy", "det_n_det.npy", "det_mask_logits.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    for f in files:
        assert np.load(tmp_path / f).dtype in (np.float32, np.float64), f
    # small arrays whole and exact (integers as float64)
    assert (np.load(tmp_path / "ids.npy") == step["ids"].numpy()).all() and np.load(tmp_path / "ids.npy").dtype == np.float64
    assert (np.load(tmp_path / "z.npy") == step["z"].numpy()).all()
    # the crops (75 MB as float32) are a sorted row sample; the rows file names them
    rows = np.load(tmp_path / "crops_rows.npy").astype(np.int64)
    assert written["crops"][0] == len(rows) < 256 and (np.diff(rows) > 0).all()
    assert (np.load(tmp_path / "crops.npy") == step["crops"].numpy()[rows].astype(np.float32)).all()


def test_dump_outputs_same_sample_every_time(tmp_path):
    bench = _bench()
    bench.dump_outputs(_step(), str(tmp_path / "a"))
    bench.dump_outputs(_step(), str(tmp_path / "b"))
    for f in sorted(os.listdir(tmp_path / "a")):
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all(), f


def test_dump_outputs_large_rows_fall_back_to_elements(tmp_path):
    bench = _bench()
    written = bench.dump_outputs({"big": torch.zeros((2, 5_000_000))}, str(tmp_path), limit=8 << 20)
    assert len(written["big"]) == 1 and os.path.getsize(tmp_path / "big.npy") + os.path.getsize(tmp_path / "big_rows.npy") <= 8 << 20
