#!/usr/bin/env python3
"""Time of one loss call of the soft-Dice loss driver at 2 x 13 x 128^3.

    python scripts/time_weighted_loss.py [--calls 20] [--warmup 3] [--kinds swin,unet3d,nnunet]
                                         [--package DIR] [--out DIR]

One call = statistics pass, finaliser and gradient pass (logits and dlogits [2, 128, 128, 128,
13] fp32 channel-last, int64 labels with 3 % ignored): spff_swin_loss, spff_unet3d_loss (class
weights and per-voxel weights with 30 % zeros, dice_weight 0.3) and spff_nnunet_loss, one after
the other in the same process, each timed with device events around every call; the median of
the calls after the warm-up is reported, with the bytes the two passes must move (logits twice,
labels twice, dlogits once, plus the voxel weights twice) over that time.

``--package DIR`` times the innovative3D package under DIR instead of this tree's (another
build of the library, e.g. the parent commit's, for ``--kinds swin``).  The work runs in a
fresh child process under its own time limit.  Prints one JSON line and writes it to
DIR/time_weighted_loss.json (default bench_out/weighted_loss).  Needs a ROCm device: there is
no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
B, K, S = 2, 13, 128
LIMIT_S = 240


def run(kinds, calls, warmup, package):
    sys.path.insert(0, package)
    import torch
    from innovative3D import _engine as E
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_weighted_loss: no ROCm device (there is no CPU fallback)")
    dev = "cuda"
    g = torch.Generator().manual_seed(11)
    lcl = (2.0 * torch.randn(B, S, S, S, K, generator=g)).to(dev)
    y = torch.randint(0, K, (B, S, S, S), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.03] = 255
    u = torch.rand(y.shape, generator=g) + 0.25
    u[torch.rand(y.shape, generator=g) < 0.3] = 0.0
    y, u, cw = y.to(dev), u.to(dev), torch.linspace(0.5, 2.0, K).to(dev)
    V = y.numel()
    fns = {
        "swin": (lambda: E.swin_loss_forward(lcl, y, K, 255, False, 0.5), 0),
        "unet3d": (lambda: E.unet3d_loss_forward(lcl, y, K, 255, cw, u, False, 0.7, 0.3), 8),
        "nnunet": (lambda: E.nnunet_loss_forward(lcl, y, K, 255, False, 1.0, 1.0), 0),
    }
    out = {"shape": [B, K, S, S, S], "calls": calls, "warmup": warmup,
           "device": torch.cuda.get_device_name(0), "library": str(E.lib_path())}
    for kind in kinds:
        fn, extra = fns[kind]
        for _ in range(warmup):
            out4, _dl = fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(calls)]
        for a, b in ev:
            a.record()
            out4, _dl = fn()
            b.record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        nbytes = V * (3 * 4 * K + 2 * 8 + extra)
        med = statistics.median(ms)
        out[kind] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                     "bytes_per_voxel": nbytes // V, "gb_per_s": nbytes / (med * 1e6),
                     "out4": [float(v) for v in out4.cpu()]}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="swin,unet3d,nnunet")
    ap.add_argument("--package", default=str(ROOT / "spff-unet-spcct_amd"))
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "weighted_loss"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    kinds = [k for k in a.kinds.split(",") if k]
    if a.calls < 20 or not kinds or set(kinds) - {"swin", "unet3d", "nnunet"}:
        ap.error("--calls must be >= 20 and --kinds a list of swin, unet3d, nnunet")
    if a.child:
        run(kinds, a.calls, a.warmup, a.package)
        return 0
    cmd = [sys.executable, __file__, "--child", "--calls", str(a.calls), "--warmup", str(a.warmup),
           "--kinds", ",".join(kinds), "--package", a.package]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"time_weighted_loss: exceeded {LIMIT_S} s; stopping", file=sys.stderr)
        return 124
    sys.stderr.write(r.stderr[-4000:])
    if r.returncode != 0:
        print(f"time_weighted_loss: failed ({r.returncode})", file=sys.stderr)
        return r.returncode or 1
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    print(line, flush=True)
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "time_weighted_loss.json").write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
