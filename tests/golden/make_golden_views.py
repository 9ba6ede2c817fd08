#!/usr/bin/env python3
"""Generate the prediction-view fixtures (tests/golden/views_*.npz) by running the
REFERENCE's own ``_prediction_views_and_mip`` (train.py:649-671) on the CPU.
Container-only tooling; run once:

    python tests/golden/make_golden_views.py

The reference's train.py cannot be imported offline (its module top needs pandas,
matplotlib, scikit-learn and Lightning), so the two functions that matter are compiled from
the reference file when this script runs: ``_prediction_views_and_mip`` and the
module-level ``_softmax_over_classes`` (train.py:611-614, the same lines as the nested
softmax), which gives the per-class maximum over depth that the former does not return.
None of the reference's text is stored; only arrays are.

Every file holds, stacked over the batch:
  logits [B, K, D, H, W] fp32                    the input
  center_pred, summary_pred, alpha_center, mip_pred   the reference's four outputs (fp32 run)
  mip_prob                                        max over depth of its fp32 softmax
  center_pred64, alpha_center64, mip_prob64, mip_pred64   the same on the fp64 logits
  e32_alpha, e32_mip                              max |fp32 - fp64| of the reference itself
  block_w                                         columns [0, block_w) are the saturated block
  mip_tie_share, center_tie_share                 share of all pixels that lie outside the
      block and whose top two fp64 values (of mip_prob64, of the centre row's softmax) are
      closer than 1e-5 -- the pixels a class-map comparison has to leave out

Logits: N(0, s^2) everywhere but in the left third of W, where every voxel holds +40 at one
random class and -20 elsewhere: every fp32 softmax there is exactly 1.0, so mip_prob holds
several exact 1.0s and the lowest class present along depth must win.
"""
from __future__ import annotations

import ast
import json
import os
import pathlib

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REF = pathlib.Path(os.environ.get("SPFF_REFERENCE", "/root/reference"))
LIMIT = 1 << 20  # bytes: the largest file the repository commits
TIE = 1e-5

#        name            B   K   D   H   W    s   seed  what
CASES = [("views_k13_d5", 2, 13, 5, 24, 20, 3.0, 711, "the registry depth, odd D (centre index 2)"),
         ("views_ragged", 1, 4, 7, 9, 33, 2.0, 702, "extents that fill no wave or tile"),
         ("views_k32_d3", 1, 32, 3, 8, 8, 6.0, 703, "the largest K"),
         ("views_deep", 1, 13, 64, 16, 16, 1.0, 704, "few pixels, much depth: automatic split > 1"),
         ("views_d1", 1, 3, 1, 8, 16, 4.0, 705, "D = 1, centre index 0; also the 4-D input")]


def _reference_functions(*names):
    """The named module-level functions of the reference's train.py, compiled from its file."""
    path = REF / "train.py"
    tree = ast.parse(path.read_text(), filename=str(path))
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return [ns[n] for n in names]


def _logits(rng, B, K, D, H, W, s):
    lg = (s * rng.standard_normal((B, K, D, H, W))).astype(np.float32)
    bw = W // 3
    win = rng.integers(0, K, size=(B, D, H, bw))
    for c in range(K):
        lg[:, c, :, :, :bw] = np.where(win == c, np.float32(40.0), np.float32(-20.0))
    return lg, bw


def _top2_gap(p):
    """p [K, H, W] -> the gap of the two largest values per pixel (inf when K == 1)"""
    if p.shape[0] < 2:
        return np.full(p.shape[1:], np.inf)
    t = np.sort(p, axis=0)
    return t[-1] - t[-2]


def _case(views, softmax, lg, bw):
    B, K, D, H, W = lg.shape
    out = {k: [] for k in ("center_pred", "summary_pred", "alpha_center", "mip_pred", "mip_prob",
                           "center_pred64", "alpha_center64", "mip_prob64", "mip_pred64")}
    ties = {"mip": 0, "center": 0}
    for b in range(B):
        l32, l64 = lg[b], lg[b].astype(np.float64)
        cp, sp, al, mp = views(l32)
        assert al.dtype == np.float32
        prob = np.stack([softmax(l32[:, z]) for z in range(D)], axis=1).max(axis=1)
        assert prob.dtype == np.float32 and np.array_equal(prob.argmax(axis=0), mp)
        cp64, sp64, al64, mp64 = views(l64)
        soft64 = [softmax(l64[:, z]) for z in range(D)]
        prob64 = np.stack(soft64, axis=1).max(axis=1)
        assert al64.dtype == np.float64 and np.array_equal(prob64.argmax(axis=0), mp64)
        assert np.array_equal(sp, mp) and np.array_equal(sp64, mp64)
        # the reference's fp32 class maps are its fp64 ones, and the block resolves to the
        # lowest class present along depth with an exact 1.0
        assert np.array_equal(cp, cp64) and np.array_equal(mp, mp64)
        if bw:
            lowest = l32[:, :, :, :bw].argmax(axis=0).min(axis=0)
            assert np.array_equal(mp[:, :bw], lowest)
            assert np.all(prob[:, :, :bw].max(axis=0) == np.float32(1.0))
            assert np.all(al[:, :bw] == np.float32(1.0))
        outside = np.ones((H, W), dtype=bool)
        outside[:, :bw] = False
        ties["mip"] += int(((_top2_gap(prob64) < TIE) & outside).sum())
        ties["center"] += int(((_top2_gap(soft64[D // 2]) < TIE) & outside).sum())
        for k, v in (("center_pred", cp), ("summary_pred", sp), ("alpha_center", al),
                     ("mip_pred", mp), ("mip_prob", prob), ("center_pred64", cp64),
                     ("alpha_center64", al64), ("mip_prob64", prob64), ("mip_pred64", mp64)):
            out[k].append(v)
    d = {k: np.stack(v) for k, v in out.items()}
    for k in ("center_pred", "summary_pred", "mip_pred", "center_pred64", "mip_pred64"):
        d[k] = d[k].astype(np.uint8)
    d["logits"] = lg
    d["block_w"] = np.array(bw, dtype=np.int64)
    d["e32_alpha"] = np.array(np.abs(d["alpha_center"].astype(np.float64) - d["alpha_center64"]).max())
    d["e32_mip"] = np.array(np.abs(d["mip_prob"].astype(np.float64) - d["mip_prob64"]).max())
    d["mip_tie_share"] = np.array(ties["mip"] / (B * H * W))
    d["center_tie_share"] = np.array(ties["center"] / (B * H * W))
    return d


def main():
    views, softmax = _reference_functions("_prediction_views_and_mip", "_softmax_over_classes")
    for name, B, K, D, H, W, s, seed, what in CASES:
        rng = np.random.default_rng(seed)
        lg, bw = _logits(rng, B, K, D, H, W, s)
        d = _case(views, softmax, lg, bw)
        assert d["mip_tie_share"] <= 0.005 and d["center_tie_share"] <= 0.005, name
        d["meta"] = np.array(json.dumps(dict(B=B, K=K, D=D, H=H, W=W, s=s, seed=seed, what=what)))
        path = HERE / f"{name}.npz"
        np.savez_compressed(path, **d)
        size = path.stat().st_size
        print(f"wrote {path.name} ({size / 1024:.0f} KiB)  e32_alpha={float(d['e32_alpha']):.3g} "
              f"e32_mip={float(d['e32_mip']):.3g}  tie shares mip={float(d['mip_tie_share']):.4f} "
              f"center={float(d['center_tie_share']):.4f}")
        assert size < LIMIT, (path.name, size)


if __name__ == "__main__":
    main()
