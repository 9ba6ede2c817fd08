#!/usr/bin/env python3
"""Generate the R2UNet3D parity fixtures (tests/golden/r2u_*.npz) by running the
REFERENCE's own LitR2UNet3D_Published on the CPU, under the stub harness of
make_golden.py.  Container-only tooling; run once:

    python tests/golden/make_golden_r2u.py

Every fixture stores inputs and outputs, so no test needs the reference:
logits, the module's Dice-only loss and dice, ``loss_unified``
(ce_plus_macro_dice_loss of the same logits), parameter gradients (full up to
16 384 elements, else head / tail / sum), state-dict shapes, parameter names,
and the reference's own fp32-vs-fp64 logit error and argmax flip count.
Parameters come from innovative3D.weightgen.synth_state(seed).

The file names do not start with "fx": tests/_golden.fixture_names() globs
fx*.npz for the SPFF family.
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

FULL_MAX = 16384


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


def _run(torch, Hh, lit, x_np, y_np, K, seed, grads=True):
    sd = _load_synth(torch, lit, seed)
    lit.train()
    lit.zero_grad(set_to_none=True)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    ign = lit.hparams.ignore_index
    logits = lit(x)
    loss, dice = lit._dice_only_loss_with_logits(logits, y, ignore_index=ign)
    out = {"x": x_np, "labels": y_np,
           "logits": logits.detach().numpy().astype(np.float32),
           "loss": np.array(float(loss.detach()), dtype=np.float64),
           "dice": np.array(float(dice), dtype=np.float64)}
    with torch.no_grad():
        lu = Hh.ce_plus_macro_dice_loss(logits.detach(), y, K, ignore_index=255)
    out["loss_unified"] = np.array(float(lu), dtype=np.float64)
    names = [k for k, _p in lit.named_parameters()]
    if grads:
        loss.backward()
        for k, p in lit.named_parameters():
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            G._summ(out, k, g.detach().numpy().astype(np.float32), FULL_MAX)
    # the reference's own fp32 error: the same module in fp64
    l64 = copy.deepcopy(lit).double()
    with torch.no_grad():
        lg64 = l64(x.double())
    out["ref_err32"] = np.array(float((lg64 - logits.detach().double()).abs().max()))
    out["ref_flips32"] = np.array(int((lg64.argmax(1) != logits.detach().argmax(1)).sum()))
    if grads:
        l64.zero_grad(set_to_none=True)
        ls64, _ = l64._dice_only_loss_with_logits(l64(x.double()), y, ignore_index=ign)
        ls64.backward()
        n32 = np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in lit.parameters()))
        n64 = np.sqrt(sum(float((p.grad ** 2).sum()) for p in l64.parameters()))
        out["ref_gradnorm_rel32"] = np.array(abs(n32 - n64) / n64)
    out["param_names"] = np.array(names)
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array(json.dumps({k: list(v.shape) for k, v in sd.items()}))
    return out


def _loss_case(torch, M, rng, shape, K, ignore, empty):
    """One loss-only case: logits, labels, loss, dice and the fp64 dlogits."""
    B = shape[0]
    lg = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, K, size=(B,) + tuple(shape[2:])).astype(np.int64)
    if ignore is not None:
        y[rng.random(y.shape) < 0.05] = ignore
    for b in empty:  # samples without foreground: background and ignored voxels only
        y[b] = np.where(y[b] == (ignore if ignore is not None else -1), y[b], 0)
    fn = M.LitR2UNet3D_Published._dice_only_loss_with_logits
    t = torch.from_numpy(lg).double().requires_grad_(True)
    loss, dice = fn(t, torch.from_numpy(y), ignore_index=ignore)
    if loss.requires_grad:
        loss.backward()
        dl = t.grad.numpy()
    else:
        dl = np.zeros(shape, dtype=np.float64)
    l32, d32 = fn(torch.from_numpy(lg), torch.from_numpy(y), ignore_index=ignore)
    return {"logits": lg, "labels": y, "loss": np.array(float(loss)), "dice": np.array(float(dice)),
            "loss32": np.array(float(l32)), "dice32": np.array(float(d32)), "dlogits": dl,
            "ignore": np.array(-1 if ignore is None else ignore), "K": np.array(K)}


def main():
    C, M, Hh = G._import_reference()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cases = {}
    cls = M.LitR2UNet3D_Published

    # --- the registry factory: K 13, base 16, t 2; D pad 5 -> 16, bottleneck 1 x 2 x 2 ---
    _name, factory, _dm, _ck = [v for v in C.VARIANTS if v[0] == "R2UNet3D"][0]
    torch.manual_seed(0)
    lit = factory()
    reg_kw = dict(num_classes=13, in_channels=1, base_features=16, t=2, lr=1e-3, weight_decay=0.0,
                  ignore_index=255, pad_multiple=16)
    _fill_hparams(lit, cls, reg_kw)
    rng = np.random.default_rng(301)
    x = rng.standard_normal((1, 1, 5, 32, 32)).astype(np.float32)
    y = G._labels(rng, (1, 5, 32, 32), 13)
    cases["r2u_registry_k13"] = dict(
        meta=dict(variant="R2UNet3D", in_ch=1, base=16, K=13, t=2, seed=21, ignore_index=255,
                  pad_multiple=16, lit=True, hparams={k: lit.hparams[k] for k in sorted(lit.hparams)}),
        data=_run(torch, Hh, lit, x, y, 13, 21))

    # --- base 8, t 3, K 5, batch 2; sample 1 has no foreground ---
    kw = dict(num_classes=5, in_channels=1, base_features=8, t=3, ignore_index=255)
    torch.manual_seed(0)
    lit = cls(**kw)
    _fill_hparams(lit, cls, kw)
    rng = np.random.default_rng(302)
    # (inputs on a 1/16 grid: the stored fp32 array compresses to a quarter, which keeps
    #  the file under the repository's 1 MiB limit for a committed file)
    x = (np.round(rng.standard_normal((2, 1, 16, 32, 32)) * 16) / 16).astype(np.float32)
    y = G._labels(rng, (2, 16, 32, 32), 5)
    y[1] = np.where(y[1] == 255, 255, 0)
    cases["r2u_core_b8_t3"] = dict(
        meta=dict(variant="R2UNet3D", in_ch=1, base=8, K=5, t=3, seed=22, ignore_index=255,
                  pad_multiple=16, lit=True),
        data=_run(torch, Hh, lit, x, y, 5, 22))

    # --- H / W padding and crop: logits, loss and dice only ---
    torch.manual_seed(0)
    lit = cls(**reg_kw)
    _fill_hparams(lit, cls, reg_kw)
    rng = np.random.default_rng(303)
    x = rng.standard_normal((1, 1, 5, 24, 40)).astype(np.float32)
    y = G._labels(rng, (1, 5, 24, 40), 13)
    cases["r2u_pad_hw"] = dict(
        meta=dict(variant="R2UNet3D", in_ch=1, base=16, K=13, t=2, seed=23, ignore_index=255,
                  pad_multiple=16, lit=True),
        data=_run(torch, Hh, lit, x, y, 13, 23, grads=False))
    G._write(cases)

    # --- loss only: four cases in one file ---
    rng = np.random.default_rng(304)
    lc = {"a": _loss_case(torch, M, rng, (3, 13, 3, 7, 9), 13, 255, empty=[1]),
          "b": _loss_case(torch, M, rng, (2, 2, 2, 5, 5), 2, 255, empty=[]),
          "c": _loss_case(torch, M, rng, (2, 13, 3, 7, 9), 13, 255, empty=[0, 1]),
          "d": _loss_case(torch, M, rng, (2, 5, 2, 6, 7), 5, None, empty=[])}
    d = {f"{c}/{k}": v for c, cc in lc.items() for k, v in cc.items()}
    d["cases"] = np.array(sorted(lc))
    path = HERE / "r2u_loss_small.npz"
    np.savez_compressed(path, **d)
    print(f"wrote {path.name} ({path.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
