#!/usr/bin/env python3
"""Generate the fixtures of the voxel-weighted 3DUNet loss and of the nnU-Net Dice + CE loss
(tests/golden/unet3d_loss_small.npz, nnunet_loss_small.npz) by running the REFERENCE's own
functions on the CPU, under the stub harness of make_golden.py.  Container-only tooling; run
once:

    python tests/golden/make_golden_wloss.py

  3DUNet   LitCicek3DUNet_DepthAdapter_Published._loss_and_log (its _weighted_softmax_ce and
           _dice_loss): ``ce`` is the unscaled CE term, ``dice`` the Dice loss term
  nnU-Net  models.dice_ce_loss: ``ce`` is F.cross_entropy, ``dice`` the mean Dice
           (1 - soft_dice_loss_from_logits)

Every case stores its inputs and the reference's fp32 results (loss32, ce32, dice32,
dlogits32).  The fp64 results (loss, ce, dice, dlogits) are stored where the reference can
produce them: the 3DUNet wrapper casts its class weights with .float(), so with class weights
set it runs in fp32 only (``has64`` = 0).  ``use_ignore`` = 0: ignore_index None.
The wrapper also sums the denominator of its voxel-weighted CE in fp32 always; the voxel weights
are chosen so that this sum is exact (or below the clamp at 1).
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as G  # noqa: E402

LIMIT = 1 << 20  # bytes: the largest file the repository commits


def _inputs(rng, shape, K, ignore, absent=None, bg_samples=()):
    lg = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, K, size=(shape[0],) + tuple(shape[2:])).astype(np.int64)
    if absent is not None:
        y[y == absent] = (absent + 1) % K
    if ignore is not None and ignore >= 0:
        y[rng.random(y.shape) < 0.05] = ignore
    for b in bg_samples:  # a sample that is background throughout (and valid)
        y[b] = 0
    assert ((y != ignore).sum() if ignore is not None else y.size) > 0
    return lg, y


def _common(lg, y, K, ignore, include_bg, cw, dw):
    return {"logits": lg, "labels": y, "K": np.array(K),
            "use_ignore": np.array(int(ignore is not None)),
            "ignore": np.array(0 if ignore is None else ignore),
            "include_bg": np.array(int(include_bg)), "ce_weight": np.array(float(cw)),
            "dice_weight": np.array(float(dw))}


def _unet3d_case(torch, M, rng, shape, K, ignore, class_w=None, voxel="none", include_bg=False,
                 cw=1.0, dw=0.0, absent=None, bg_samples=()):
    lg, y = _inputs(rng, shape, K, ignore, absent, bg_samples)
    vw = None
    if voxel != "none":
        # on a 1/64 grid: the wrapper sums its denominator sum m u in fp32 whatever the logits'
        # dtype, and a sum of such weights is exact there, so its fp64 run is fp64 throughout
        vw = (np.round(rng.random(y.shape) * 64) / 64 + 0.25).astype(np.float32)
        if voxel == "sparse":   # sparse annotation: about 30 % of the voxels carry no weight
            vw[rng.random(y.shape) < 0.3] = 0.0
        if voxel == "tiny":     # sum m u < 1: the clamp branch of the denominator
            vw *= np.float32(0.5 / vw.sum())
            assert vw[y != ignore].sum() < 1.0
    lit = M.LitCicek3DUNet_DepthAdapter_Published(
        num_classes=K, ignore_index=ignore, class_weights=class_w, ce_weight=cw, dice_weight=dw,
        include_bg_in_dice=include_bg, voxel_weight_key="weight" if vw is not None else None)
    yt = torch.from_numpy(y)
    vt = None if vw is None else torch.from_numpy(vw)

    def run(dtype):
        t = torch.from_numpy(lg).to(dtype).requires_grad_(True)
        loss = lit._loss_and_log(t, yt, "train", vt, log_metrics=False)
        loss.backward()
        with torch.no_grad():
            ce, dice = lit._weighted_softmax_ce(t, yt, vt), lit._dice_loss(t, yt)
        return float(loss.detach()), float(ce), float(dice), t.grad.numpy()
    out = _common(lg, y, K, ignore, include_bg, cw, dw)
    if class_w is not None:
        out["class_weights"] = np.asarray(class_w, np.float32)
    if vw is not None:
        out["voxel_weights"] = vw
    l32, c32, d32, g32 = run(torch.float32)
    out.update(loss32=np.array(l32), ce32=np.array(c32), dice32=np.array(d32), dlogits32=g32,
               has64=np.array(int(class_w is None)))
    if class_w is None:
        l64, c64, d64, g64 = run(torch.float64)
        out.update(loss=np.array(l64), ce=np.array(c64), dice=np.array(d64), dlogits=g64)
    return out


def _nnunet_case(torch, M, Hh, rng, shape, K, ignore=-1, include_bg=False, cw=1.0, dw=1.0,
                 absent=None, registry=False):
    lg, y = _inputs(rng, shape, K, ignore, absent)
    yt = torch.from_numpy(y)
    F = torch.nn.functional

    def run(dtype):
        t = torch.from_numpy(lg).to(dtype).requires_grad_(True)
        loss = M.dice_ce_loss(t, yt, K, ignore_index=ignore, ce_weight=cw, dice_weight=dw,
                              include_background=include_bg)
        loss.backward()
        with torch.no_grad():
            ce = F.cross_entropy(t, yt, ignore_index=ignore)
            dice = 1.0 - M.soft_dice_loss_from_logits(t, yt, K, ignore_index=ignore,
                                                      include_background=include_bg)
        return float(loss.detach()), float(ce), float(dice), t.grad.numpy()
    out = _common(lg, y, K, ignore, include_bg, cw, dw)
    l32, c32, d32, g32 = run(torch.float32)
    l64, c64, d64, g64 = run(torch.float64)
    out.update(loss32=np.array(l32), ce32=np.array(c32), dice32=np.array(d32), dlogits32=g32,
               has64=np.array(1), loss=np.array(l64), ce=np.array(c64), dice=np.array(d64),
               dlogits=g64)
    if registry:  # the registry entry is dice_ce_loss with its own weights and background
        assert (cw, dw, include_bg) == (1.0, 1.0, False)
        r = Hh.LOSS_REGISTRY["dice_ce_nnunet"](torch.from_numpy(lg), yt, K, ignore)
        assert float(r) == l32
    return out


def _save(name, lc):
    d = {f"{c}/{k}": v for c, cc in lc.items() for k, v in cc.items()}
    d["cases"] = np.array(sorted(lc))
    path = HERE / name
    np.savez_compressed(path, **d)
    print(f"wrote {path.name} ({path.stat().st_size / 1024:.0f} KiB)")
    assert path.stat().st_size < LIMIT, (path.name, path.stat().st_size)


def main():
    _C, M, Hh = G._import_reference()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cw13 = [0.5, 1.5, 2.0, 1.0, 0.75, 1.25, 3.0, 0.25, 1.0, 0.6, 1.8, 0.9, 1.1]

    rng = np.random.default_rng(501)
    _save("unet3d_loss_small.npz", {
        "a": _unet3d_case(torch, M, rng, (3, 13, 3, 7, 9), 13, 255, class_w=cw13, voxel="sparse",
                          cw=0.7, dw=0.3),
        "b": _unet3d_case(torch, M, rng, (2, 2, 2, 5, 5), 2, 255, voxel="tiny", dw=0.0),
        "c": _unet3d_case(torch, M, rng, (2, 5, 2, 6, 7), 5, None, include_bg=True, cw=1.0, dw=1.0),
        "d": _unet3d_case(torch, M, rng, (2, 13, 3, 7, 9), 13, 255, class_w=cw13, include_bg=True,
                          cw=0.5, dw=0.5, absent=7, bg_samples=[1]),
        "e": _unet3d_case(torch, M, rng, (1, 32, 2, 4, 9), 32, 255, voxel="dense", cw=1.0, dw=0.5)})

    rng = np.random.default_rng(502)
    _save("nnunet_loss_small.npz", {
        "a": _nnunet_case(torch, M, Hh, rng, (3, 13, 3, 7, 9), 13, 255, registry=True),
        "b": _nnunet_case(torch, M, Hh, rng, (2, 2, 2, 5, 5), 2, 255),
        "c": _nnunet_case(torch, M, Hh, rng, (2, 5, 2, 6, 7), 5, -1, include_bg=True, cw=0.3,
                          dw=1.7),
        "d": _nnunet_case(torch, M, Hh, rng, (2, 13, 3, 7, 9), 13, 255, absent=7),
        "e": _nnunet_case(torch, M, Hh, rng, (1, 32, 2, 4, 9), 32, 255)})


if __name__ == "__main__":
    main()
