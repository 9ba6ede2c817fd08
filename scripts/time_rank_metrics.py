#!/usr/bin/env python3
"""Time of spff_rank_auc (csrc/rank.hip), the exact PR-AUC / ROC-AUC ranking pass of the test
step, at the registry's test shapes.

    python scripts/time_rank_metrics.py [--calls 20] [--warmup 3] [--out DIR]

Synthetic logits 1 x 13 x 5 x 512 x 512 and 2 x 13 x 5 x 512 x 512 (channel-last on the device,
3 % of the labels 255), logits mode, both ``per_sample`` settings.  Each case: warm-up calls,
then >= 20 calls each between two device events on the stream; the median is reported, with
the minimum and maximum.  The workspace and the output are allocated once, outside the events:
the call itself allocates nothing and never synchronises.

Next to the time, the bytes the radix design must move at the least -- four passes that
each read and write every 4-byte key (passes x 8 B x keys) plus one read of the logits --
and the bytes the kernels as built move (the key store, the labels, a histogram read of the
keys per pass for segments of more than one tile, the curve pass's reads).  ``floor_ms`` is
the least bytes over the HBM peak of 8 TB/s (spec); ``fraction_of_floor`` is floor_ms over the
measured median.  There is no pass threshold.

Prints one JSON line per case and writes them to DIR/time_rank_metrics.json (default
bench_out/rank_metrics).  Needs a ROCm device: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

K, VOL = 13, (5, 512, 512)
HBM_PEAK = 8.0e12  # bytes / s, spec
PASSES = 4


def traffic(B, V, per_sample):
    """(keys, least bytes, bytes as built): see the module docstring."""
    n = B * V
    keys = K * n if per_sample else (2 * K - 1) * n
    logits = 4 * K * n
    least = PASSES * 8 * keys + logits
    seg_max = V if per_sample else (K - 1) * n
    multi = seg_max > 4096  # some segment has more than one tile
    built = (logits + 8 * n            # rows and labels read once
             + 4 * keys                # key store
             + PASSES * 8 * keys       # scatter: read + write
             + (PASSES * 4 * keys if multi else 0)  # histogram read per pass
             + (2 if multi else 1) * 4 * keys)      # curve: tile totals, then the terms
    return keys, least, built


def case(B, per_sample, calls, warmup, check=False):
    import ctypes

    import torch
    from innovative3D import _engine as E
    V = VOL[0] * VOL[1] * VOL[2]
    g = torch.Generator().manual_seed(11)
    logits = (3.0 * torch.randn((B, V, K), generator=g)).to("cuda")
    y = torch.randint(0, K, (B, V), generator=g)
    y[torch.rand((B, V), generator=g) < 0.03] = 255
    y = y.to("cuda")
    L = E.lib()
    ws_bytes = int(L.spff_rank_auc_ws_bytes(B, V, K, int(per_sample)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rows = B * K if per_sample else K + 1
    out = torch.empty((rows, 4), dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        E.check(L.spff_rank_auc(E._ptr(logits), E._ptr(y), B, V, K, 1, int(per_sample),
                                E._ptr(out), E._ptr(ws), stream), "spff_rank_auc")

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(calls)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    o = out.cpu()
    check_diff = None
    if check:
        # the sort and the scans at this size against the numpy definition, on the same
        # fp32 scores (scores mode: identical tie structure, so 1e-9 as in the tests)
        import numpy as np
        sys.path.insert(0, str(ROOT / "tests"))
        import _rank_oracle as RO
        scores = torch.softmax(logits, dim=2)
        got = E.rank_auc(scores, y, K, False, per_sample).cpu().numpy()
        want = RO.rank_rows(scores.cpu().numpy(), y.cpu().numpy(), K, per_sample)
        assert np.array_equal(got[:, 2:], want[:, 2:]), "n_pos / n_neg differ from the oracle"
        assert np.array_equal(np.isnan(got), np.isnan(want))
        check_diff = float(np.nanmax(np.abs(got[:, :2] - want[:, :2])))
        assert check_diff <= 1e-9, check_diff
    keys, least, built = traffic(B, V, per_sample)
    med = statistics.median(ms)
    floor_ms = least / HBM_PEAK * 1e3
    return {"shape": [B, K, *VOL], "per_sample": bool(per_sample), "from_logits": True,
            "calls": calls, "warmup": warmup, "device": torch.cuda.get_device_name(0),
            "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
            "keys": keys, "workspace_bytes": ws_bytes,
            "least_bytes": least, "built_bytes": built, "floor_ms": floor_ms,
            "fraction_of_floor": floor_ms / med, "built_TBps": built / (med * 1e-3) / 1e12,
            "rows_finite": int(torch.isfinite(o[:, :2]).all(1).sum()), "rows": rows,
            "oracle_max_abs_diff": check_diff,
            "roc_auc_mean": float(torch.nanmean(o[:, 1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true",
                    help="also compare the batch-1 cases with the numpy oracle (host sorts: ~10 s)")
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "rank_metrics"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20")
    import torch
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_rank_metrics: no ROCm device (there is no CPU fallback)")
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []
    for B in (1, 2):
        for per_sample in (False, True):
            r = case(B, per_sample, a.calls, a.warmup, a.check and B == 1)
            print(json.dumps(r), flush=True)
            lines.append(r)
    (out / "time_rank_metrics.json").write_text("\n".join(json.dumps(l) for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
