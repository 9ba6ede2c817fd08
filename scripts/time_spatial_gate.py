#!/usr/bin/env python3
"""Step time of the SPCT core's spatial attention and gated skips at the headline shape.

    python scripts/time_spatial_gate.py [--rounds 8] [--warmup 2] [--out DIR]
    rocprofv3 --kernel-trace --stats -d DIR/prof -o sa -- \\
        python scripts/time_spatial_gate.py --phase prof [--steps 5]
    python scripts/time_spatial_gate.py --phase table --stats DIR/prof/.../sa_kernel_stats.csv

One step = forward + CE / hard-Dice loss + backward of build_spct_energyfilm_fourier
(K 13, base 32, 5 input channels, f16x3) on a 2 x 5 x 128^3 batch.

  time   four modules in one process -- both flags off, use_spatial, use_skip_gate, both --
         warmed up, then ROUNDS rounds that run one step of each in turn, every step timed
         with device events: median and minimum ms per variant and the added ms per flag.
  prof   STEPS steps of the module with both flags on, for a kernel trace taken from outside
         (the profiler runs this phase as its own process; counters are never collected
         together with a trace).
  table  the new kernels' compulsory HBM bytes per step, computed here from the shapes, over
         their times in a rocprofv3 kernel-stats file of a prof run: GB/s per kernel.

Prints one JSON line per phase and writes it to DIR (default bench_out/spatial_gate).  Needs
a ROCm device for time / prof: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

SHAPE = (2, 5, 128, 128, 128)
K, BASE = 13, 32
VARIANTS = {"off": (False, False), "spatial": (True, False), "gate": (False, True),
            "both": (True, True)}


def _model(spatial, gate):
    import numpy as np
    import torch
    import innovative3D.models as M
    from innovative3D.weightgen import synth_state
    core = M.build_spct_energyfilm_fourier(num_classes=K, base=BASE, in_channels=SHAPE[1],
                                           use_spatial=spatial, use_skip_gate=gate)
    for b in core._blocks():
        b.fgate._ensure_mask(SHAPE[2], "cpu")
    st = synth_state([(k, tuple(v.shape)) for k, v in core.state_dict().items()], seed=5,
                     mask_jitter=0.25)
    core.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    core.math = "f16x3"
    return core.to("cuda")


def _batch():
    import torch
    g = torch.Generator().manual_seed(7)
    x = torch.randn(SHAPE, generator=g).to("cuda")
    y = torch.randint(0, K, (SHAPE[0],) + SHAPE[2:], generator=g)
    y[torch.rand(y.shape, generator=g) < 0.03] = 255
    return x, y.to("cuda")


def _step(core, x, y):
    import innovative3D.helpers as Hh
    for p in core.parameters():
        p.grad = None
    loss, _conf = Hh.ce_dice_with_confusion(core(x), y, K, 255)
    loss.backward()
    return loss


def phase_time(rounds, warmup):
    import torch
    x, y = _batch()
    mods = {n: _model(*fl) for n, fl in VARIANTS.items()}
    for _ in range(warmup):
        for m in mods.values():
            _step(m, x, y)
    torch.cuda.synchronize()
    ms = {n: [] for n in mods}
    for _ in range(rounds):
        for n, m in mods.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _step(m, x, y)
            b.record()
            b.synchronize()
            ms[n].append(a.elapsed_time(b))
    out = {"phase": "time", "shape": SHAPE, "rounds": rounds}
    for n, v in ms.items():
        out[n] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    for n in ("spatial", "gate", "both"):
        out["added_ms_" + n] = out[n]["median_ms"] - out["off"]["median_ms"]
    return out


def phase_prof(steps):
    import torch
    x, y = _batch()
    m = _model(True, True)
    for _ in range(steps):
        _step(m, x, y)
    torch.cuda.synchronize()
    return {"phase": "prof", "steps": steps}


def kernel_bytes():
    """compulsory HBM bytes per step of each new kernel (both flags on), from the shapes:
    every operand read once, every result written once, fp32"""
    B, _, D, H, W = SHAPE
    out = {}

    def add(k, n):
        out[k] = out.get(k, 0) + 4 * n
    for lvl in range(4):  # enc1, enc2, enc3, bott
        V, C = B * D * (H >> lvl) * (W >> lvl), BASE << lvl
        tiles = B * D * -(-(H >> lvl) // 16) * -(-(W >> lvl) // 16)
        add("k_sa_stats", V * (C + 3))            # z; map (2) + idx
        add("k_sa_stencil_fwd", V * 3)            # map; a
        add("k_sa_scale", V * (2 * C + 1))        # z, a; e
        add("k_sa_bwd_dot", V * (2 * C + 2))      # de, z, a; dt
        add("k_sa_stencil_bwd", V * 5 + tiles * 294)  # dt, map; dm, partial rows
        add("k_sa_bwd_dx", V * (2 * C + 4))       # de, a, dm, idx; dz
    for lvl in range(3):  # g1, g2, g3
        M, C = B * D * (H >> lvl) * (W >> lvl), BASE << lvl
        hid = C // 2
        add("k_ag_fwd", M * (2 * hid + 1 + 2 * C))    # hidden rw, psi, up, s
        add("k_ag_bwd_vox", M * (4 * C + 2))          # ds, up, dd rw, psi, dpp
        add("k_ag_wpsi_part", M * (hid + 1))
        add("k_ag_dhid", M * (2 * hid + 1))
    return out


def phase_table(stats, steps):
    byt = kernel_bytes()
    rows = {}
    with open(stats, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            tot = r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or r.get("TotalDuration")
            if not tot:
                continue
            for k in list(byt) + ["k_act_apply"]:
                if k + "(" in name or name.endswith(k) or ("::" + k) in name or name == k:
                    e = rows.setdefault(k, {"ns": 0.0, "calls": 0})
                    e["ns"] += float(tot)
                    e["calls"] += int(float(r.get("Calls", 0) or 0))
    out = {"phase": "table", "steps": steps, "kernels": {}}
    for k, e in rows.items():
        rec = {"ms_per_step": e["ns"] / steps / 1e6, "calls_per_step": e["calls"] / steps}
        if k in byt:
            rec["MB_per_step"] = byt[k] / 1e6
            rec["GB_per_s"] = byt[k] * steps / e["ns"]
        out["kernels"][k] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=("time", "prof", "table"), default="time")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "spatial_gate"))
    a = ap.parse_args()
    if a.phase == "time":
        res = phase_time(a.rounds, a.warmup)
    elif a.phase == "prof":
        res = phase_prof(a.steps)
    else:
        if not a.stats:
            ap.error("--phase table needs --stats FILE")
        res = phase_table(a.stats, a.steps)
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"time_spatial_gate_{a.phase}.json").write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
