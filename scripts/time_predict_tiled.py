#!/usr/bin/env python3
"""Time of sliding-window inference on the engine, and of its blend against torch ops.

    python scripts/time_predict_tiled.py [--rounds 3] [--calls 2] [--warmup 1] [--out DIR]

One 5 x 256^3 volume, windows of 128^3 at overlap 0.5 (27 windows), base 32, K 13, f16x3,
synthetic weights and labels (3 % of them 255).  Device events around whole calls:

  call   ``core.predict_tiled(x, roi, labels=y, ignore_index=255)``: 27 forwards on the
         forward-only plan plus gather, blend, class map and counts.

The blend alone, on the logits the last forward left in one buffer (their values do not
change what moves), in one process, alternating for >= 3 rounds:

  H  per window spff_tile_gather and spff_tile_accumulate, then spff_tile_finalize with
     labels (csrc/tile.hip);
  T  the same blend with torch ops: per window a slice copy into the staging tensor and one
     ``addcmul_`` of the permuted logits and the 3-D weight into a strided view of a
     channel-first [K, D, H, W] accumulator, then ``argmax`` to uint8.  The leanest torch
     form: no count map, no division, no confusion counts.

Reported: ms per call of every round, medians, T's round-to-round spread (the resolution of
the comparison) and ``H_within_T_spread`` = median(H) <= median(T) + spread(T); the three
kernels timed by themselves (27 gathers, 27 accumulates, one finalize between two events),
their sum as a share of the call, and for each the bytes it must move over its time against
the 6.29 TB/s copy rate measured on the MI355X.

Prints one JSON line and writes it to DIR/time_predict_tiled.json (default bench_out/tiled).
Run it once more under ``rocprofv3 --kernel-trace --stats -- python ...`` (no counters) for
the per-kernel times.  Needs a ROCm device: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

VOL, CIN, ROI, OVERLAP, K, BASE, MATH = (256, 256, 256), 5, (128, 128, 128), 0.5, 13, 32, "f16x3"
COPY_RATE = 6.29e12  # bytes / s, the measured device copy rate


def timed(fn, calls):
    """ms per call of ``calls`` back-to-back calls between two device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "tiled"))
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be >= 3")
    import torch
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_predict_tiled: no ROCm device (there is no CPU fallback)")
    import innovative3D.models as M
    from innovative3D import _engine as E
    from innovative3D import tiling as T
    from innovative3D.weightgen import synth_state

    core = M.build_spct_energyfilm_fourier(num_classes=K, base=BASE, in_channels=CIN)
    for b in core._blocks():
        b.fgate._ensure_mask(ROI[0], "cpu")
    st = synth_state([(k, tuple(v.shape)) for k, v in core.state_dict().items()], seed=13,
                     mask_jitter=0.25)
    core.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    core = core.to("cuda").eval()
    core.math = MATH
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, CIN, *VOL, generator=g).cuda()
    y = torch.randint(0, K, (1,) + VOL, generator=g)
    y[torch.rand((1,) + VOL, generator=g) < 0.03] = 255
    y = y.cuda()
    table = T.window_table(VOL, ROI, OVERLAP)
    nwin, V, RV = len(table), VOL[0] * VOL[1] * VOL[2], ROI[0] * ROI[1] * ROI[2]

    def call():
        return core.predict_tiled(x, ROI, overlap=OVERLAP, labels=y, ignore_index=255)

    for _ in range(a.warmup):
        mask, conf = call()
    torch.cuda.synchronize()
    t_call = [timed(call, a.calls) for _ in range(a.rounds)]

    # the blend alone, on one window-output buffer
    plan = core._infer_plan
    stage = torch.empty((1, CIN) + ROI, device="cuda")
    tiles = plan.forward(E.tile_gather(x[0], table[:1], ROI, out=stage), core._flat)
    w = tuple(torch.from_numpy(T.axis_weights(r)).cuda() for r in ROI)
    acc = torch.zeros(VOL + (K,), device="cuda")
    hmask = torch.empty(VOL, dtype=torch.uint8, device="cuda")
    hconf = torch.empty(K * (K + 1), dtype=torch.int64, device="cuda")
    w3 = ((w[0][:, None, None] * w[1][None, :, None]) * w[2][None, None, :]).contiguous()
    tiles_cf = tiles[0].permute(3, 0, 1, 2)  # the view torch blends from
    acc_cf = torch.zeros((K,) + VOL, device="cuda")
    rows = [table[i:i + 1] for i in range(nwin)]
    starts = [tuple(int(v) for v in r[0, :3]) for r in rows]

    def gathers():
        for r in rows:
            E.tile_gather(x[0], r, ROI, out=stage)

    def accumulates():
        for r in rows:
            E.tile_accumulate(tiles, r, w, acc)

    def finalize():
        E.tile_finalize(acc, labels=y[0], ignore_index=255, mask=hmask, conf=hconf)

    def blend_h():
        acc.zero_()
        for r in rows:
            E.tile_gather(x[0], r, ROI, out=stage)
            E.tile_accumulate(tiles, r, w, acc)
        finalize()

    def blend_t():
        acc_cf.zero_()
        for z, yy, xx in starts:
            stage.copy_(x[:, :, z:z + ROI[0], yy:yy + ROI[1], xx:xx + ROI[2]])
            acc_cf[:, z:z + ROI[0], yy:yy + ROI[1], xx:xx + ROI[2]].addcmul_(tiles_cf, w3)
        return acc_cf.argmax(0).to(torch.uint8)

    for _ in range(max(1, a.warmup)):
        blend_h()
        tmask = blend_t()
    torch.cuda.synchronize()
    same = bool(torch.equal(tmask, hmask))
    n = max(3, a.calls)
    th, tt = [], []
    for _ in range(a.rounds):
        th.append(timed(blend_h, n))
        tt.append(timed(blend_t, n))
    t_g, t_a, t_f = timed(gathers, n), timed(accumulates, n), timed(finalize, n)
    by_g = nwin * 2 * 4 * CIN * RV            # window read + staging write
    by_a = nwin * (4 * K * RV + 2 * 4 * K * RV)  # tile read, acc read + write
    by_f = V * (4 * K + 8 + 1)                # acc and labels read, mask written

    def kern(ms, nbytes):
        return {"ms": ms, "bytes": nbytes, "TBps": nbytes / (ms * 1e-3) / 1e12,
                "of_copy_rate": nbytes / (ms * 1e-3) / COPY_RATE}

    mc, mh, mt = statistics.median(t_call), statistics.median(th), statistics.median(tt)
    spread = max(tt) - min(tt)
    r = {"volume": [CIN] + list(VOL), "roi": list(ROI), "overlap": OVERLAP, "windows": nwin,
         "base": BASE, "K": K, "math": MATH, "device": torch.cuda.get_device_name(0),
         "rounds": a.rounds, "calls": a.calls, "plan_layout": plan.layout,
         "plan_workspace_bytes": plan.ws_bytes, "conf_total": int(conf.sum()),
         "call_ms_rounds": t_call, "call_ms": mc,
         "H_ms_rounds": th, "T_ms_rounds": tt, "H_ms": mh, "T_ms": mt, "T_spread_ms": spread,
         "H_minus_T_ms": mh - mt, "H_within_T_spread": bool(mh <= mt + spread),
         "masks_equal": same,
         "kernels": {"k_tile_gather": kern(t_g, by_g), "k_tile_accumulate": kern(t_a, by_a),
                     "k_tile_finalize": kern(t_f, by_f)},
         "tile_kernels_ms": t_g + t_a + t_f, "tile_kernels_share_of_call": (t_g + t_a + t_f) / mc}
    print(json.dumps(r), flush=True)
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "time_predict_tiled.json").write_text(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
