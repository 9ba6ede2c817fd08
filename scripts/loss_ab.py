#!/usr/bin/env python3
"""Bitwise A/B of the loss entry points between two builds of the library.

    python scripts/loss_ab.py OUT_DIR LIB_A [LIB_B]     (LIB_B default: the in-tree library)

Each library runs in a fresh child process (SPFF_LIB) under its own time limit: spff_swin_loss
on the four cases of tests/test_gpu_swin.py, spff_r2u_dice_loss on r2u_loss_small a-d,
spff_rupp_loss on rupp_loss_small a-e, spff_loss and spff_loss_ex on one K = 13 case; out4,
dlogits and conf of every case go to OUT_DIR/loss_<a|b>.npz.  The parent then compares the
two files array by array (np.array_equal, NaN positions equal), prints one line per array,
writes the lines to OUT_DIR/compare.txt and exits non-zero on any difference.  Needs a ROCm
device: there is no fallback."""
from __future__ import annotations

import os
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "tests", ROOT / "spff-unet-spcct_amd", ROOT):
    sys.path.insert(0, str(p))
LIMIT_S = 240


def run(out: pathlib.Path) -> None:
    import torch
    import innovative3D._engine as E
    from test_gpu_swin import LOSS_CASES, loss_case

    dev, res = "cuda", {}

    def cl(a):
        return E.to_channels_last(torch.as_tensor(a).to(dev))

    def keep(name, out4, dl, conf=None):
        torch.cuda.synchronize()
        res[name + "/out4"], res[name + "/dlogits"] = out4.cpu().numpy(), dl.cpu().numpy()
        if conf is not None:
            res[name + "/conf"] = conf.cpu().numpy()

    for c in sorted(LOSS_CASES):
        lg, y, K, include_bg, w = loss_case(c)
        keep(f"swin/{c}", *E.swin_loss_forward(cl(lg), y.to(dev), K, 255, include_bg, w))
    z = np.load(ROOT / "tests/golden/r2u_loss_small.npz")
    for c in "abcd":
        ign = int(z[f"{c}/ignore"])
        keep(f"r2u/{c}", *E.r2u_dice_loss_forward(
            cl(z[f"{c}/logits"]), torch.as_tensor(z[f"{c}/labels"]).to(dev), int(z[f"{c}/K"]),
            None if ign < 0 else ign))
    z = np.load(ROOT / "tests/golden/rupp_loss_small.npz")
    for c in "abcde":
        ign = int(z[f"{c}/ignore"])
        keep(f"rupp/{c}", *E.rupp_loss_forward(
            cl(z[f"{c}/logits"]), torch.as_tensor(z[f"{c}/labels"]).to(dev), int(z[f"{c}/K"]),
            None if ign < 0 else ign, bool(int(z[f"{c}/include_bg"])),
            float(z[f"{c}/ce_weight"]), float(z[f"{c}/dice_weight"])))
    g = torch.Generator().manual_seed(5)
    K, shape = 13, (2, 5, 24, 40)
    lg = cl(3.0 * torch.randn(shape[0], K, *shape[1:], generator=g))
    y = torch.randint(0, K, shape, generator=g)
    y[torch.rand(shape, generator=g) < 0.05] = 255
    keep("ce_dice/k13", *E.ce_dice_forward(lg, y.to(dev), K, 255, 1e-6))
    cw = torch.linspace(0.5, 2.0, K)
    keep("weighted_ce/k13", *E.weighted_ce_forward(lg, y.to(dev), K, 255, cw))
    cnt = torch.tensor([2 * int((y != 255).sum())], device=dev)
    keep("weighted_ce/k13_count", *E.weighted_ce_forward(lg, y.to(dev), K, 255, None,
                                                         count_override=cnt))
    np.savez(out, **res)
    print(f"{E.lib_path()}: {len(res)} arrays -> {out}")


def main() -> int:
    out_dir = pathlib.Path(sys.argv[1])
    out_dir.mkdir(parents=True, exist_ok=True)
    libs = [pathlib.Path(a).resolve() for a in sys.argv[2:4]]
    files = []
    for tag, lib in zip("ab", libs + [None] * (2 - len(libs))):
        env = dict(os.environ)
        env.pop("SPFF_LIB", None)
        if lib is not None:
            env["SPFF_LIB"] = str(lib)
        files.append(out_dir / f"loss_{tag}.npz")
        r = subprocess.run([sys.executable, __file__, "--run", str(files[-1])], env=env,
                           timeout=LIMIT_S)
        if r.returncode:
            print(f"child {tag} exited with {r.returncode}; nothing more is started")
            return r.returncode
    a, b = (np.load(f) for f in files)
    lines = [f"a = {sys.argv[2]}",
             f"b = {sys.argv[3] if len(libs) > 1 else 'the in-tree library'}"]
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        same = np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") and \
            a[k].dtype == b[k].dtype
        lines.append(f"{k:32s} {a[k].dtype} {tuple(a[k].shape)}  "
                     f"{'bitwise equal' if same else 'DIFFERENT'}")
        if not same:
            bad.append(k)
    lines.append(f"{len(a.files)} arrays, {len(bad)} different or missing: {bad}")
    (out_dir / "compare.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--run":
        run(pathlib.Path(sys.argv[2]))
    else:
        sys.exit(main())
