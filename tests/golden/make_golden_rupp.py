#!/usr/bin/env python3
"""Generate the ResUNet++ parity fixtures (tests/golden/rupp_*.npz) by running the
REFERENCE's own LitResUNetPP3D_Published on the CPU, under the stub harness of
make_golden.py.  Container-only tooling; run once:

    python tests/golden/make_golden_rupp.py

Every fixture stores inputs and outputs, so no test needs the reference: logits, the
module's loss, macro dice and CE (dice_ce_loss_with_metrics), ``loss_unified``
(ce_plus_macro_dice_loss of the same logits), parameter gradients (full up to the case's
threshold, else head / tail / sum), state-dict shapes, parameter names, and the
reference's own fp32-vs-fp64 logit error and argmax flip count.  Parameters come from
innovative3D.weightgen.synth_state(seed).

The file names do not start with "fx": tests/_golden.fixture_names() globs fx*.npz for
the SPFF family.
"""
from __future__ import annotations

import copy
import inspect
import json
import os
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as G  # noqa: E402

LIMIT = 1 << 20  # bytes: the largest file the repository commits


def _fill_hparams(lit, cls, kwargs):
    """The stub save_hyperparameters() records explicit arguments only: fill in the
    constructor's values (defaults overridden by ``kwargs``) as Lightning would."""
    sig = inspect.signature(cls.__init__)
    for n, p in sig.parameters.items():
        if n == "self":
            continue
        lit.hparams[n] = kwargs[n] if n in kwargs else p.default


def _load_synth(torch, lit, seed):
    sd = lit.state_dict()
    st = G._synth_state([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    lit.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    return sd


def _grid16(a):
    """Inputs on a 1/16 grid: the stored fp32 array compresses to about a quarter."""
    return (np.round(a * 16) / 16).astype(np.float32)


def _run(torch, Hh, lit, x_np, y_np, K, seed, grads=True, full_max=16384):
    sd = _load_synth(torch, lit, seed)
    lit.train()
    lit.zero_grad(set_to_none=True)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    logits = lit(x)
    loss, dice, ce = lit._loss(logits, y)
    out = {"x": x_np, "labels": y_np,
           "logits": logits.detach().numpy().astype(np.float32),
           "loss": np.array(float(loss.detach()), dtype=np.float64),
           "dice": np.array(float(dice), dtype=np.float64),
           "ce": np.array(float(ce), dtype=np.float64)}
    with torch.no_grad():
        lu = Hh.ce_plus_macro_dice_loss(logits.detach(), y, K, ignore_index=255)
    out["loss_unified"] = np.array(float(lu), dtype=np.float64)
    names = [k for k, _p in lit.named_parameters()]
    if grads:
        loss.backward()
        for k, p in lit.named_parameters():
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            G._summ(out, k, g.detach().numpy().astype(np.float32), full_max)
    # the reference's own fp32 error: the same module in fp64
    l64 = copy.deepcopy(lit).double()
    with torch.no_grad():
        lg64 = l64(x.double())
    out["ref_err32"] = np.array(float((lg64 - logits.detach().double()).abs().max()))
    out["ref_flips32"] = np.array(int((lg64.argmax(1) != logits.detach().argmax(1)).sum()))
    if grads:
        l64.zero_grad(set_to_none=True)
        ls64, _d, _c = l64._loss(l64(x.double()), y)
        ls64.backward()
        n32 = np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in lit.parameters()))
        n64 = np.sqrt(sum(float((p.grad ** 2).sum()) for p in l64.parameters()))
        out["ref_gradnorm_rel32"] = np.array(abs(n32 - n64) / n64)
    out["param_names"] = np.array(names)
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array(json.dumps({k: list(v.shape) for k, v in sd.items()}))
    return out


def _loss_case(torch, M, rng, shape, K, ignore, include_bg=False, absent=None, bg_samples=(),
               cw=0.5, dw=0.5):
    """One loss-only case: logits, labels, and the fp64 loss, dice, ce and dlogits."""
    B = shape[0]
    lg = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, K, size=(B,) + tuple(shape[2:])).astype(np.int64)
    if absent is not None:
        y[y == absent] = (absent + 1) % K
    if ignore is not None:
        y[rng.random(y.shape) < 0.05] = ignore
    for b in bg_samples:  # a sample that is background throughout (and valid)
        y[b] = 0
    assert ((y != ignore).sum() if ignore is not None else y.size) > 0
    fn = M.dice_ce_loss_with_metrics
    kw = dict(ignore_index=ignore, include_bg_in_dice=include_bg, ce_weight=cw, dice_weight=dw)
    t = torch.from_numpy(lg).double().requires_grad_(True)
    loss, dice, ce = fn(t, torch.from_numpy(y), K, **kw)
    loss.backward()
    l32, d32, c32 = fn(torch.from_numpy(lg), torch.from_numpy(y), K, **kw)
    return {"logits": lg, "labels": y, "loss": np.array(float(loss)), "dice": np.array(float(dice)),
            "ce": np.array(float(ce)), "loss32": np.array(float(l32)),
            "dice32": np.array(float(d32)), "ce32": np.array(float(c32)),
            "dlogits": t.grad.numpy(), "ignore": np.array(-1 if ignore is None else ignore),
            "K": np.array(K), "include_bg": np.array(int(include_bg)),
            "ce_weight": np.array(cw), "dice_weight": np.array(dw)}


def main():
    C, M, Hh = G._import_reference()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cases = {}
    cls = M.LitResUNetPP3D_Published

    # --- the registry factory: K 13, base 16; D pad 5 -> 16, bottleneck 1 x 2 x 2 ---
    _name, factory, _dm, _ck = [v for v in C.VARIANTS if v[0] == "ResUNet++"][0]
    torch.manual_seed(0)
    lit = factory()
    reg_kw = dict(num_classes=13, in_channels=1, base_features=16, include_bg_in_dice=False,
                  ce_weight=0.5, dice_weight=0.5, lr=1e-4, weight_decay=1e-5, ignore_index=255,
                  pad_multiple=16)
    _fill_hparams(lit, cls, reg_kw)
    rng = np.random.default_rng(401)
    x = rng.standard_normal((1, 1, 5, 32, 32)).astype(np.float32)
    y = G._labels(rng, (1, 5, 32, 32), 13)
    cases["rupp_registry_k13"] = dict(
        meta=dict(variant="ResUNet++", in_ch=1, base=16, K=13, seed=31, ignore_index=255,
                  pad_multiple=16, lit=True, hparams={k: lit.hparams[k] for k in sorted(lit.hparams)}),
        data=_run(torch, Hh, lit, x, y, 13, 31, full_max=8192))

    # --- base 8, K 5, batch 2: batch-pooled Dice differs from per-sample Dice ---
    kw = dict(num_classes=5, in_channels=1, base_features=8, ignore_index=255)
    torch.manual_seed(0)
    lit = cls(**kw)
    _fill_hparams(lit, cls, kw)
    rng = np.random.default_rng(402)
    x = _grid16(rng.standard_normal((2, 1, 16, 32, 32)))
    y = G._labels(rng, (2, 16, 32, 32), 5)
    cases["rupp_core_b8"] = dict(
        meta=dict(variant="ResUNet++", in_ch=1, base=8, K=5, seed=32, ignore_index=255,
                  pad_multiple=16, lit=True),
        data=_run(torch, Hh, lit, x, y, 5, 32, full_max=4096))

    # --- bottleneck 1 x 1 x 10: every dilation up to 8 has off-centre taps inside ---
    kw = dict(num_classes=3, in_channels=1, base_features=8, ignore_index=255)
    torch.manual_seed(0)
    lit = cls(**kw)
    _fill_hparams(lit, cls, kw)
    rng = np.random.default_rng(403)
    x = _grid16(rng.standard_normal((1, 1, 16, 16, 160)))
    y = G._labels(rng, (1, 16, 16, 160), 3)
    cases["rupp_aspp_wide"] = dict(
        meta=dict(variant="ResUNet++", in_ch=1, base=8, K=3, seed=33, ignore_index=255,
                  pad_multiple=16, lit=True),
        data=_run(torch, Hh, lit, x, y, 3, 33, full_max=4096))
    g3 = lit.backbone.b_aspp.branches[3].weight.grad.detach().numpy()
    off = np.abs(g3).reshape(g3.shape[0], g3.shape[1], 27)
    assert off[:, :, 12].max() > 0 and off[:, :, 14].max() > 0, "dilation 8 off-centre taps dead"

    # --- H / W padding and crop: logits, loss and dice only ---
    torch.manual_seed(0)
    lit = cls(**reg_kw)
    _fill_hparams(lit, cls, reg_kw)
    rng = np.random.default_rng(404)
    x = rng.standard_normal((1, 1, 5, 24, 40)).astype(np.float32)
    y = G._labels(rng, (1, 5, 24, 40), 13)
    cases["rupp_pad_hw"] = dict(
        meta=dict(variant="ResUNet++", in_ch=1, base=16, K=13, seed=34, ignore_index=255,
                  pad_multiple=16, lit=True),
        data=_run(torch, Hh, lit, x, y, 13, 34, grads=False))
    G._write(cases)

    # --- loss only: five cases in one file ---
    rng = np.random.default_rng(405)
    lc = {"a": _loss_case(torch, M, rng, (2, 13, 3, 7, 9), 13, 255, absent=7),
          "b": _loss_case(torch, M, rng, (2, 2, 2, 5, 5), 2, 255),
          "c": _loss_case(torch, M, rng, (2, 5, 2, 6, 7), 5, None),
          "d": _loss_case(torch, M, rng, (2, 13, 3, 7, 9), 13, 255, include_bg=True),
          "e": _loss_case(torch, M, rng, (3, 5, 3, 5, 6), 5, 255, bg_samples=[1], cw=0.3, dw=0.7)}
    d = {f"{c}/{k}": v for c, cc in lc.items() for k, v in cc.items()}
    d["cases"] = np.array(sorted(lc))
    path = HERE / "rupp_loss_small.npz"
    np.savez_compressed(path, **d)
    print(f"wrote {path.name} ({path.stat().st_size / 1024:.0f} KiB)")
    for p in sorted(HERE.glob("rupp_*.npz")):
        assert p.stat().st_size < LIMIT, (p.name, p.stat().st_size)


if __name__ == "__main__":
    main()
