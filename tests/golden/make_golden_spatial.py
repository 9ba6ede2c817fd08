#!/usr/bin/env python3
"""Generate the spatial-attention / gated-skip parity fixtures (tests/golden/spa_*.npz,
gate_*.npz) by running the REFERENCE's own UNet3D_SpectralCore with use_spatial /
use_skip_gate on the CPU, under the stub harness of make_golden.py.  Container-only
tooling; run once:

    python tests/golden/make_golden_spatial.py

Every fixture stores inputs and outputs, so no test needs the reference: logits, CE, the
hard-Dice loss part, the loss, parameter gradients (full up to FULL_MAX elements, else head /
tail / sum), state-dict shapes and parameter names.  Its meta also records the reference's
own fp32-vs-fp64 logit error and argmax flip count, and the smallest relative top-2 gap of
the channel max at every ``sa`` stage's input; the generator asserts at most 2 flips and no
gap below 1e-5 (choose another seed otherwise).  Parameters come from
innovative3D.weightgen.synth_state(seed).

The file names do not start with "fx": tests/_golden.fixture_names() globs fx*.npz into the
parity tests of the plans without these flags.
"""
from __future__ import annotations

import copy
import json
import os
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as G  # noqa: E402

LIMIT = 1 << 20   # bytes: the largest file the repository commits
FULL_MAX = 4096   # gradients above this many elements are summarised
NAMES = ("spa_full_b8", "spa_only_d1", "spa_ragged_hw", "gate_only_cin5", "spa_lit_k13")


def _sa_gaps(torch, core, run):
    """smallest (top1 - top2) / max|z| of the channel max at each sa stage's input"""
    gaps, hooks = {}, []
    for i, mod in enumerate(core.sa):
        if isinstance(mod, torch.nn.Identity):
            continue

        def pre(_m, args, i=i):
            z = args[0].detach()
            t = torch.topk(z, 2, dim=1).values
            gaps[i] = float(((t[:, 0] - t[:, 1]) / z.abs().max().clamp_min(1e-30)).min())
        hooks.append(mod.register_forward_pre_hook(pre))
    run()
    for h in hooks:
        h.remove()
    return [gaps[i] for i in sorted(gaps)]


def _run(torch, Hh, model, core, x_np, y_np, K, seed, jitter):
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    with torch.no_grad():
        model(x)  # creates the lazy FourierGate masks
    sd = model.state_dict()
    st = G._synth_state([(k, tuple(v.shape)) for k, v in sd.items()], seed, jitter)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    model.zero_grad(set_to_none=True)
    logits = model(x)
    ce = torch.nn.functional.cross_entropy(logits, y, ignore_index=255)
    dice_part = Hh.macro_dice_loss(logits, y, K, 255, 1e-6)
    loss = Hh.ce_plus_macro_dice_loss(logits, y, K, ignore_index=255)
    loss.backward()
    out = {"x": x_np, "labels": y_np, "logits": logits.detach().numpy().astype(np.float32),
           "ce": np.array(ce.item(), dtype=np.float64),
           "dice_loss": np.array(dice_part, dtype=np.float64),
           "loss": np.array(loss.item(), dtype=np.float64)}
    names, seen = [], set()
    for k, p in model.named_parameters(remove_duplicate=False):
        if id(p) in seen:  # ``_mask`` and ``freq_mask`` alias one tensor
            continue
        seen.add(id(p))
        names.append(k)
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        G._summ(out, k, g.detach().numpy().astype(np.float32), FULL_MAX)
    out["param_names"] = np.array(names)
    out["state_keys"] = np.array(list(sd.keys()))
    out["state_shapes"] = np.array(json.dumps({k: list(v.shape) for k, v in sd.items()}))
    # the reference's own fp32 error: the same module in fp64
    m64 = copy.deepcopy(model).double()
    for mod in m64.modules():  # EnergyFiLM3D builds its positional code in fp32
        if isinstance(getattr(mod, "mlp", None), torch.nn.Sequential):
            mod.mlp.register_forward_pre_hook(lambda _m, a: (a[0].double(),))
    with torch.no_grad():
        lg64 = m64(x.double())
        gaps = _sa_gaps(torch, core, lambda: model(x))
    extra = {"ref_err32": float((lg64 - logits.detach().double()).abs().max()),
             "ref_flips32": int((lg64.argmax(1) != logits.detach().argmax(1)).sum()),
             "sa_min_gap": gaps}
    assert extra["ref_flips32"] <= 2, extra
    assert all(g >= 1e-5 for g in gaps), extra
    return out, extra


def main():
    C, M, Hh = G._import_reference()
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cases = {}

    def add(name, model, core, shape, K, seed, rng_seed, jitter, **meta):
        rng = np.random.default_rng(rng_seed)
        x = rng.standard_normal(shape).astype(np.float32)
        y = G._labels(rng, (shape[0],) + tuple(shape[2:]), K)
        data, extra = _run(torch, Hh, model, core, x, y, K, seed, jitter)
        cases[name] = dict(meta=dict(variant="SPFF-UNet", in_ch=shape[1], K=K, seed=seed,
                                     jitter=jitter, **meta, **extra), data=data)
        print(name, extra)

    # levels 24x40 ... 3x5: a stencil wider than the plane at the bottleneck; gate hidden
    # widths 16, 8 and 4
    torch.manual_seed(0)
    core = M.build_spct_energyfilm_fourier(num_classes=4, base=8, use_spatial=True,
                                           use_skip_gate=True)
    add("spa_full_b8", core, core, (2, 1, 5, 24, 40), 4, 41, 501, 0.25, base=8, lit=False,
        efilm=True, fgate=True, se=True, specse=True, spatial=True, skip_gate=True)

    # D = 1: only the centre depth plane of the 3-deep kernel is ever inside; extents 16, 8,
    # 4, 2 (at 8 x 8 the bottleneck is one voxel per instance and the reference's
    # InstanceNorm3d refuses it: "Expected more than 1 spatial element when training")
    torch.manual_seed(0)
    core = M.UNet3D_SpectralCore(in_channels=1, num_classes=2, base=8, ksd=3, use_spatial=True)
    add("spa_only_d1", core, core, (1, 1, 1, 16, 16), 2, 42, 502, 0.0, base=8, lit=False,
        efilm=False, fgate=False, se=False, specse=False, spatial=True, skip_gate=False)

    # odd pooled extents (18 -> 9 -> 4, 20 -> 10 -> 5 -> 2): the separate pool pass and the
    # _cat resize, both reading the attended output
    torch.manual_seed(0)
    core = M.UNet3D_SpectralCore(in_channels=5, num_classes=3, base=8, ksd=3, use_se=True,
                                 use_specse=True, use_spatial=True)
    add("spa_ragged_hw", core, core, (1, 5, 2, 18, 20), 3, 43, 503, 0.0, base=8, lit=False,
        efilm=False, fgate=False, se=True, specse=True, spatial=True, skip_gate=False)

    # gated skips alone, 5 input channels
    torch.manual_seed(0)
    core = M.UNet3D_SpectralCore(in_channels=5, num_classes=5, base=16, ksd=3,
                                 use_skip_gate=True)
    add("gate_only_cin5", core, core, (2, 5, 3, 16, 8), 5, 48, 508, 0.0, base=16, lit=False,
        efilm=False, fgate=False, se=False, specse=False, spatial=False, skip_gate=True)

    # the Lit module: ``model.``-prefixed keys, labels with ignore voxels
    torch.manual_seed(0)
    lit = M.LitSPCT_EFiLM_FourierGate(num_classes=13, base=8, use_spatial=True,
                                      use_skip_gate=True)
    add("spa_lit_k13", lit, lit.model, (2, 1, 5, 16, 16), 13, 45, 505, 0.25, base=8, lit=True,
        efilm=True, fgate=True, se=True, specse=True, spatial=True, skip_gate=True)

    assert sorted(cases) == sorted(NAMES)
    G._write(cases)
    for n in NAMES:
        p = HERE / f"{n}.npz"
        assert p.stat().st_size < LIMIT, (p.name, p.stat().st_size)


if __name__ == "__main__":
    main()
