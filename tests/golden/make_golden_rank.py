#!/usr/bin/env python3
"""Generate the ranking-metric fixtures (tests/golden/rank_*.npz) by running the
REFERENCE's own ``BaseLitModel._shared_step(batch, "test")`` on the CPU, under the stub
harness of make_golden.py, with scikit-learn doing the work as in the reference.
Container-only tooling; run once:

    python tests/golden/make_golden_rank.py

The module under test is the reference's BaseLitModel with a one-line ``model`` that hands
back the stored logits; every ``self.log`` call is captured.  The step runs once on the
whole batch (keys ``log/<name>``) and once per single sample (``log_s<b>/<name>``: the
per-volume expectations).  Each file also stores the logits, the labels, the fp32 softmax
scores the reference ranked, ``sklearn.__version__`` and the reference's own rounding
sensitivity: the same step on the fp64 logits (``d64/...``, ``d64_s<b>/...``) and, per
metric, the largest absolute difference to the fp32 run (``ref_d64/<metric>``).

The file names do not start with "fx": tests/_golden.fixture_names() globs fx*.npz for
the SPFF family.
"""
from __future__ import annotations

import json
import math
import pathlib
import sys
import warnings

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as G  # noqa: E402

LIMIT = 1 << 20  # bytes: the largest file the repository commits
METRICS = ("pr_auc", "roc_auc", "iou", "precision")


def _metric_of(key):
    """'test_pr_auc_class_3' -> 'pr_auc'; None for the dice / sens / spec / loss keys."""
    for m in METRICS:
        if key.startswith(f"test_{m}_"):
            return m
    return None


def _step(torch, M, logits, labels, K):
    """Every value the reference logs in one test step on (logits, labels)."""
    lit = M.BaseLitModel(num_classes=K)
    lit.model = lambda x: x  # the batch's "image" is the stored logits
    rec = {}
    lit.log = lambda name, value, **kw: rec.__setitem__(name, float(value))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lit._shared_step((logits, labels), "test")
    return rec


def _case(torch, M, logits_np, labels_np, K):
    import sklearn
    lg, y = torch.from_numpy(logits_np), torch.from_numpy(labels_np)
    B = lg.shape[0]
    out = {"logits": logits_np, "labels": labels_np,
           "scores": torch.softmax(lg, dim=1).numpy().astype(np.float32),
           "sklearn_version": np.array(sklearn.__version__)}
    worst = {m: 0.0 for m in METRICS}
    runs = [("", lg, y)] + [(f"_s{b}", lg[b:b + 1], y[b:b + 1]) for b in range(B)]
    keys = None
    for tag, l, t in runs:
        r32 = _step(torch, M, l, t, K)
        r64 = _step(torch, M, l.double(), t, K)
        assert len([k for k in r32 if _metric_of(k)]) == 4 * K + 8, sorted(r32)
        keys = sorted(r32)
        for k in keys:
            out[f"log{tag}/{k}"] = np.array(r32[k], dtype=np.float64)
            m = _metric_of(k)
            if m is None:
                continue
            out[f"d64{tag}/{k}"] = np.array(r64[k], dtype=np.float64)
            assert math.isnan(r32[k]) == math.isnan(r64[k]), (tag, k)
            if not math.isnan(r32[k]):
                worst[m] = max(worst[m], abs(r32[k] - r64[k]))
    for m in METRICS:
        out[f"ref_d64/{m}"] = np.array(worst[m], dtype=np.float64)
    out["keys"] = np.array(keys)
    return out


def main():
    _C, M, _Hh = G._import_reference()
    import torch
    cases = {}

    # --- tails: 192 voxels per sample, label 255 as a negative, micro and per-sample rows ---
    rng = np.random.default_rng(501)
    K = 4
    lg = (3.0 * rng.standard_normal((2, K, 3, 8, 8))).astype(np.float32)
    y = G._labels(rng, (2, 3, 8, 8), K, ignore_frac=0.10)
    cases["rank_small_k4"] = (dict(K=K, what="tails, label 255, micro, per-sample"),
                              _case(torch, M, lg, y, K))

    # --- ties: a coarse logit grid and rows saturated at +-40 (p = 1.0 and ~1e-35 exactly
    # tied); class 3 absent from the labels but predicted, class 4 absent from both ---
    rng = np.random.default_rng(502)
    K = 5
    lg = (np.round(2.0 * rng.standard_normal((2, K, 3, 8, 8))) / 2.0).astype(np.float32)
    lg[:, 4] = -30.0 - np.round(rng.random((2, 3, 8, 8)) * 4)  # never the argmax
    sat = rng.random((2, 3, 8, 8)) < 0.35
    win = rng.integers(0, 4, size=(2, 3, 8, 8))
    for c in range(K):
        lg[:, c][sat] = np.where(win[sat] == c, 40.0, -40.0)
    y = rng.integers(0, 3, size=(2, 3, 8, 8)).astype(np.int64)  # labels 0..2 only
    y[rng.random(y.shape) < 0.05] = 255
    assert (lg.argmax(1) == 3).any() and not (lg.argmax(1) == 4).any()
    cases["rank_ties_k5"] = (dict(K=K, what="exact tie groups, absent classes, NaN handling"),
                             _case(torch, M, lg.astype(np.float32), y, K))

    # --- the registry's K: 5 760 keys per pooled class segment, 69 120 in the micro one ---
    rng = np.random.default_rng(503)
    K = 13
    lg = (np.round(3.0 * rng.standard_normal((2, K, 5, 24, 24)) * 8) / 8).astype(np.float32)
    y = G._labels(rng, (2, 5, 24, 24), K)
    cases["rank_k13_multiblock"] = (dict(K=K, what="several tiles per segment"),
                                    _case(torch, M, lg, y, K))

    for name, (meta, d) in cases.items():
        d = dict(d)
        d["meta"] = np.array(json.dumps(meta))
        path = HERE / f"{name}.npz"
        np.savez_compressed(path, **d)
        size = path.stat().st_size
        print(f"wrote {path.name} ({size / 1024:.0f} KiB)  " +
              "  ".join(f"d64[{m}]={float(d['ref_d64/' + m]):.3g}" for m in METRICS))
        assert size < LIMIT, (path.name, size)


if __name__ == "__main__":
    main()
