#!/usr/bin/env python3
"""Generate the UNETR fixtures (tests/golden/unetr_*.npz) by running the REFERENCE's own
LitUNETR_Published on the CPU, under the stub harness of make_golden.py.  Container-only
tooling; run once:

    python tests/golden/make_golden_unetr.py

MONAI cannot be imported here, so before the reference's module is built a stand-in module
is put into sys.modules["monai.networks.nets"] whose ``UNETR`` is the torch module of
tests/_unetr_oracle.py (MONAI 1.5.2's constructor signature and state-dict keys, restated).
The fixtures thereby pin the REFERENCE's pad, resample, crop, loss and gradient flow (and
its keyword filtering and registry arguments); the network BODY stays unpinned.

Every fixture stores inputs and outputs, so no test needs the reference: logits, loss,
parameter gradients (full up to the case's threshold, else head / tail / sum; plus, from
the reference's fp64 run, which no fp32 rounding or LeakyReLU knife edge touches, every
gradient's sum and l2 norm and the fp32 run's largest deviation from it), state-dict shapes,
parameter names, and the reference's own fp32-vs-fp64 logit error and argmax flip count.  Parameters come from innovative3D.weightgen.synth_state(seed); inputs lie on the
1/16 grid.
"""
from __future__ import annotations

import copy
import inspect
import json
import os
import pathlib
import sys
import types

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import make_golden as G  # noqa: E402

LIMIT = 1 << 20  # bytes: the largest file the repository commits


def _install_monai_stub():
    import _unetr_oracle as U
    monai = types.ModuleType("monai")
    networks = types.ModuleType("monai.networks")
    nets = types.ModuleType("monai.networks.nets")
    nets.UNETR = U.UNETR
    monai.networks, networks.nets = networks, nets
    sys.modules.update({"monai": monai, "monai.networks": networks, "monai.networks.nets": nets})


def _fill_hparams(lit, cls, kwargs):
    sig = inspect.signature(cls.__init__)
    for n, p in sig.parameters.items():
        if n != "self":
            lit.hparams[n] = kwargs[n] if n in kwargs else p.default


def _grid16(a):
    return (np.round(a * 16) / 16).astype(np.float32)


def _run(torch, lit, x_np, y_np, seed, full_max):
    sd = lit.state_dict()
    st = G._synth_state([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    lit.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    lit.train()
    lit.zero_grad(set_to_none=True)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    logits = lit(x)
    loss = lit._loss(logits, y)
    out = {"x": x_np, "labels": y_np, "logits": logits.detach().numpy().astype(np.float32),
           "loss": np.array(float(loss.detach()), dtype=np.float64)}
    loss.backward()
    names, unused = [], []
    for k, p in lit.named_parameters():
        names.append(k)
        if p.grad is None:
            unused.append(k)
            continue
        G._summ(out, k, p.grad.detach().numpy().astype(np.float32), full_max)
    # the reference's own fp32 error: the same module in fp64
    l64 = copy.deepcopy(lit).double()
    l64.zero_grad(set_to_none=True)
    lg64 = l64(x.double())
    l64._loss(lg64, y).backward()
    lg64 = lg64.detach()
    g32 = {k: p.grad for k, p in lit.named_parameters() if p.grad is not None}
    for k, p in l64.named_parameters():
        if p.grad is not None:
            # [sum, l2 norm, max |fp32 - fp64|, max |g|] of the reference's fp64 gradient;
            # the third is the reference's own fp32 gradient error (rounding, knife edges)
            g = p.grad.detach().numpy().reshape(-1)
            e = float((g32[k].detach().double() - p.grad).abs().max())
            out["grad64/" + k] = np.array([g.sum(), np.sqrt((g ** 2).sum()), e, np.abs(g).max()])
    out["ref_err32"] = np.array(float((lg64 - logits.detach().double()).abs().max()))
    out["ref_flips32"] = np.array(int((lg64.argmax(1) != logits.detach().argmax(1)).sum()))
    out["param_names"] = np.array(names)
    out["unused_params"] = np.array(unused)
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array(json.dumps({k: list(v.shape) for k, v in sd.items()}))
    return out


def _meta(lit, K, seed, img, f, hidden, mlp, heads):
    return dict(variant="UNETR", in_ch=1, K=K, seed=seed, img=list(img), feature_size=f,
                hidden=hidden, mlp_dim=mlp, heads=heads, ignore_index=255, include_bg=False,
                ce_weight=0.5, lit=True,
                hparams={k: (list(v) if isinstance(v, tuple) else v)
                         for k, v in sorted(lit.hparams.items())})


def _loss_case(torch, lit, rng, shape, K, bg_samples=()):
    lg = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, K, size=(shape[0],) + tuple(shape[2:])).astype(np.int64)
    y[rng.random(y.shape) < 0.05] = 255
    for b in bg_samples:  # a sample without foreground
        y[b] = np.where(y[b] == 255, 255, 0)
    t = torch.from_numpy(lg).double().requires_grad_(True)
    loss = lit._loss(t, torch.from_numpy(y))
    loss.backward()
    l32 = lit._loss(torch.from_numpy(lg), torch.from_numpy(y))
    return {"logits": lg, "labels": y, "loss": np.array(float(loss)),
            "loss32": np.array(float(l32)), "dlogits": t.grad.numpy(), "K": np.array(K)}


def main():
    _install_monai_stub()
    C, M, _Hh = G._import_reference()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cls = M.LitUNETR_Published
    small = dict(feature_size=8, hidden_size=128, mlp_dim=256, num_heads=2, ignore_index=255,
                 include_bg_in_dice=False, ce_weight=0.5)
    cases = {}

    # --- no resample: the padded input is the network grid (8 tokens) ---
    kw = dict(num_classes=4, img_size=(32, 32, 32), **small)
    torch.manual_seed(0)
    lit = cls(**kw)
    _fill_hparams(lit, cls, kw)
    rng = np.random.default_rng(501)
    x = _grid16(rng.standard_normal((1, 1, 32, 32, 32)))
    y = G._labels(rng, (1, 32, 32, 32), 4)
    cases["unetr_same_k4"] = dict(meta=_meta(lit, 4, 41, (32, 32, 32), 8, 128, 256, 2),
                                  data=_run(torch, lit, x, y, 41, full_max=2048))

    # --- pad (5, 72, 40) -> (16, 80, 48); D up x3, H down 80 -> 48, W identity; 27 tokens;
    #     batch 2, 3 % ignore labels, class 3 absent ---
    kw = dict(num_classes=5, img_size=(48, 48, 48), **small)
    torch.manual_seed(0)
    lit = cls(**kw)
    _fill_hparams(lit, cls, kw)
    rng = np.random.default_rng(502)
    x = _grid16(rng.standard_normal((2, 1, 5, 72, 40)))
    y = G._labels(rng, (2, 5, 72, 40), 5, absent=3)
    cases["unetr_resample_b2"] = dict(meta=_meta(lit, 5, 42, (48, 48, 48), 8, 128, 256, 2),
                                      data=_run(torch, lit, x, y, 42, full_max=2048))

    # --- the registry factory: img 96^3, 216 tokens, 12 heads of 64 ---
    _name, factory, _dm, _ck = [v for v in C.VARIANTS if v[0] == "UNETR"][0]
    torch.manual_seed(0)
    lit = factory()
    reg_kw = dict(num_classes=13, img_size=(96, 96, 96), in_channels=1, feature_size=16,
                  hidden_size=768, mlp_dim=3072, num_heads=12, pos_embed="perceptron",
                  norm_name="instance", res_block=True, dropout_rate=0.0, lr=1e-4,
                  weight_decay=1e-2, warmup_epochs=5, use_ce_alongside_dice=True, ce_weight=0.5,
                  include_bg_in_dice=False, ignore_index=255)
    _fill_hparams(lit, cls, reg_kw)
    rng = np.random.default_rng(503)
    x = _grid16(rng.standard_normal((1, 1, 5, 48, 48)))
    y = G._labels(rng, (1, 5, 48, 48), 13)
    cases["unetr_registry_k13"] = dict(meta=_meta(lit, 13, 43, (96, 96, 96), 16, 768, 3072, 12),
                                       data=_run(torch, lit, x, y, 43, full_max=1024))
    G._write(cases)

    # --- loss only ---
    rng = np.random.default_rng(504)
    lc = {"a": _loss_case(torch, lit, rng, (2, 13, 3, 7, 9), 13),
          "b": _loss_case(torch, lit, rng, (3, 5, 3, 5, 6), 5, bg_samples=[1])}
    d = {f"{c}/{k}": v for c, cc in lc.items() for k, v in cc.items()}
    d["cases"] = np.array(sorted(lc))
    path = HERE / "unetr_loss_small.npz"
    np.savez_compressed(path, **d)
    print(f"wrote {path.name} ({path.stat().st_size / 1024:.0f} KiB)")
    for p in sorted(HERE.glob("unetr_*.npz")):
        assert p.stat().st_size < LIMIT, (p.name, p.stat().st_size)


if __name__ == "__main__":
    main()
