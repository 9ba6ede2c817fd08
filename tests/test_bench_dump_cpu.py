"""bench.py --dump-outputs: the writer (`bench.dump_outputs`) on host tensors -- whole arrays
keep their shape and values, an array above its share of the budget becomes a sample that is
the same from call to call, everything is float32 / float64 and the files stay under 64 MB.
"""
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _arrays(scale=1.0):
    g = torch.Generator().manual_seed(3)
    big = torch.randn(5_000_011, generator=g) * scale
    return {"loss": torch.tensor([2.5]), "conf": torch.arange(13 * 14).view(13, 14),
            "logits": torch.randn(2, 3, 5, 7, 11, generator=g), "grads": big}


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    # a budget the 20 MB `grads` array does not fit in: it is sampled, the others are whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1_000_000)
    arrs = _arrays()
    bench.dump_outputs(tmp_path / "a", arrs)
    bench.dump_outputs(tmp_path / "b", _arrays(scale=2.0))
    got = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert sorted(got) == ["conf", "grads", "logits", "loss"]
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [2.5]
    assert got["conf"].dtype == np.float64 and got["conf"].shape == (13, 14)
    assert np.array_equal(got["conf"], arrs["conf"].numpy())
    assert got["logits"].dtype == np.float32
    assert np.array_equal(got["logits"], arrs["logits"].numpy())
    gr = got["grads"]
    assert gr.dtype == np.float32 and gr.ndim == 1 and 0 < gr.size < arrs["grads"].numel()
    assert sum(a.nbytes for a in got.values()) <= 1_000_000
    # the sample holds elements of the array, at the same indices in every call
    assert np.isin(gr, arrs["grads"].numpy()).all()
    assert np.array_equal(np.load(tmp_path / "b" / "grads.npy"), 2.0 * gr)


def test_dump_outputs_default_budget_is_under_64_mb(tmp_path):
    g = torch.Generator().manual_seed(0)
    bench.dump_outputs(tmp_path, {"loss": torch.tensor([1.0]),
                                  "logits": torch.randn(20_000_000, generator=g)})
    files = list(tmp_path.glob("*.npy"))
    assert len(files) == 2
    assert sum(f.stat().st_size for f in files) <= 64 * 1000 * 1000
    assert np.load(tmp_path / "logits.npy").size < 20_000_000
