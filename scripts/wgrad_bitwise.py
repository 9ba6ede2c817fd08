#!/usr/bin/env python3
"""Bitwise comparison of the split-precision conv weight gradient between two libraries.

    [SPFF_LIB=other.so] python scripts/wgrad_bitwise.py run DIR    # dw of every case -> DIR/*.npy
    python scripts/wgrad_bitwise.py cmp DIR_A DIR_B                # compare two such directories

`run` computes spff_conv3d_wgrad_ld (f16x3 and bf16x6) of the cases of
tests/test_gpu_wgrad_loop.py from seeded inputs; `cmp` compares every .npy file the two
directories hold (bench.py --dump-outputs directories too) as raw bytes and exits 1 on any
difference or on a file only one of them has."""
import pathlib
import sys

import numpy as np

CASES = [
    (2, 1, 16, 16, 16, 32, 3), (2, 2, 24, 40, 16, 32, 3), (1, 5, 24, 40, 24, 48, 3),
    (2, 3, 8, 16, 5, 32, 3), (1, 7, 16, 16, 40, 13, 3), (2, 4, 16, 16, 32, 32, 1),
    (1, 130, 8, 16, 16, 32, 3),
]


def run(out):
    import torch
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "spff-unet-spcct_amd"))
    from innovative3D import _engine as E
    out.mkdir(parents=True, exist_ok=True)
    L, p, dev = E.lib(), E._ptr, torch.device("cuda")
    st = E._stream(dev)
    print("library:", E.lib_path())
    for case in CASES:
        B, D, H, W, cin, cout, ksd = case
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, D, H, W, cin, generator=g)
        lddy = (cout + 3) // 4 * 4  # (dy's channel stride: a multiple of 4, zero-filled)
        dy = torch.zeros(B, D, H, W, lddy)
        dy[..., :cout] = torch.randn(B, D, H, W, cout, generator=g)
        dy = dy.to(dev)
        ldx = (cin + 7) // 8 * 8
        xcl = torch.zeros(B, D, H, W, ldx)
        xcl[..., :cin] = x
        xcl = xcl.to(dev)
        ws = torch.empty(L.spff_conv3d_ws_bytes(B, D, H, W, cin, cout, ksd), dtype=torch.uint8,
                         device=dev)
        for mode in ("f16x3", "bf16x6"):
            dw = torch.full((cout, cin, ksd, 3, 3), float("nan"), device=dev)
            E.check(L.spff_conv3d_wgrad_ld(p(xcl), ldx, p(dy), lddy, p(dw), B, D, H, W, cin, cout,
                                           ksd, E.MATH_NAMES[mode], p(ws), st), "wgrad")
            torch.cuda.synchronize()
            np.save(out / ("dw_" + "_".join(map(str, case)) + f"_{mode}.npy"), dw.cpu().numpy())
    print("wrote", len(CASES) * 2, "arrays to", out)


def cmp(a, b):
    fa = {f.name for f in a.glob("*.npy")}
    fb = {f.name for f in b.glob("*.npy")}
    bad = sorted(fa ^ fb)
    for n in bad:
        print("only in one directory:", n)
    for n in sorted(fa & fb):
        x, y = np.load(a / n), np.load(b / n)
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        if same:
            print(f"bitwise equal  {n}  {x.shape} {x.dtype}")
        else:
            nd = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape else -1
            print(f"DIFFERENT      {n}  {x.shape} vs {y.shape}, {nd} bytes differ")
            bad.append(n)
    print(f"{len(fa & fb) - len([n for n in bad if n in fa & fb])} of {len(fa | fb)} files bitwise equal")
    return 1 if bad or not fa else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(pathlib.Path(sys.argv[2]))
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(pathlib.Path(sys.argv[2]), pathlib.Path(sys.argv[3])))
    else:
        sys.exit(__doc__)
