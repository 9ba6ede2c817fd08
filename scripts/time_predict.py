#!/usr/bin/env python3
"""Time of an evaluation step on the engine, with and without the fused class-mask head.

    python scripts/time_predict.py [--rounds 3] [--calls 10] [--warmup 3] [--out DIR]

The headline shape 2 x 5 x 128^3 (base 32, K 13, f16x3), synthetic weights and labels (3 %
of them 255).  In one process, alternating for >= 3 rounds:

  A  the logits path: the no-grad ``model(x)`` on the full layout, then ``E.confusion``
     (per_class_metrics_3d): the logits are written, then read back;
  B  ``model.predict(x, labels=y, ignore_index=255)`` on the forward-only layout: the head
     forms the class byte and the counts from the logits in its registers.

Each round: ``calls`` calls of A between two device events, then ``calls`` of B.  Reported per
path: ms per call of every round, their median, and A's round-to-round spread (max - min of
its rounds), which is the resolution of the comparison; and both plans' workspace bytes.

The head kernels by themselves (spff_debug_set key 5: the head alone on the workspace the
previous forward left), >= 20 back-to-back calls between two events: k_head_fwd_s, then
spff_confusion's pass over the stored logits (A), and k_head_mask_s without logits (B), with
the bytes each must move (4 C in, 4 K out / 4 K + 8 in / 4 C + 8 in, 1 out per voxel) and
the rate that gives.  HBM peak 8 TB/s (spec).

Prints one JSON line and writes it to DIR/time_predict.json (default bench_out/infer).  Needs
a ROCm device: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

SHAPE, K, BASE, MATH = (2, 5, 128, 128, 128), 13, 32, "f16x3"
HBM_PEAK = 8.0e12  # bytes / s, spec


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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "infer"))
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be >= 3")
    import torch
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_predict: no ROCm device (there is no CPU fallback)")
    import innovative3D.models as M
    from innovative3D import _engine as E
    from innovative3D.synthetic import synthetic_batch
    from innovative3D.weightgen import synth_state

    core = M.build_spct_energyfilm_fourier(num_classes=K, base=BASE, in_channels=SHAPE[1])
    for b in core._blocks():
        b.fgate._ensure_mask(SHAPE[2], "cpu")
    st = synth_state([(k, tuple(v.shape)) for k, v in core.state_dict().items()], seed=13,
                     mask_jitter=0.25)
    core.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    core = core.to("cuda").eval()
    core.math, core.memory = MATH, "full"
    x, y = synthetic_batch(*SHAPE, num_classes=K, ignore_frac=0.03, seed=3)
    x, y = x.to("cuda"), y.to("cuda")
    V = y.numel()

    def path_a():
        with torch.no_grad():
            logits = core(x)
        return E.confusion(logits.permute(0, 2, 3, 4, 1), y, K, 255)

    def path_b():
        return core.predict(x, labels=y, ignore_index=255)[1]

    for _ in range(a.warmup):
        ca, cb = path_a(), path_b()
    torch.cuda.synchronize()
    same = bool(torch.equal(ca, cb))
    plan_a = core._engine_plan(x, "infer")
    plan_b = core._engine_plan(x, "infer", memory="infer")
    ra, rb = [], []
    for _ in range(a.rounds):
        ra.append(timed(path_a, a.calls))
        rb.append(timed(path_b, a.calls))

    # the head kernels alone (the workspaces hold the last forward's dec1.y2)
    flat = core._flat
    logits = plan_a.forward(x, flat)
    plan_a.debug_set(5, 1)
    plan_b.debug_set(5, 1)
    n = max(20, a.calls)
    t_head = timed(lambda: plan_a.forward(x, flat, out=logits), n)
    t_conf = timed(lambda: E.confusion(logits, y, K, 255), n)
    t_mask = timed(lambda: plan_b.predict(x, flat, y, 255), n)
    t_mask_lg = timed(lambda: plan_b.predict(x, flat, y, 255, want_logits=True), n)
    plan_a.debug_set(5, 0)
    plan_b.debug_set(5, 0)
    by_head, by_conf = V * (4 * BASE + 4 * K), V * (4 * K + 8)
    by_mask, by_mask_lg = V * (4 * BASE + 8 + 1), V * (4 * BASE + 8 + 1 + 4 * K)

    def rate(nbytes, ms):
        return nbytes / (ms * 1e-3) / 1e12

    ma, mb = statistics.median(ra), statistics.median(rb)
    r = {"shape": list(SHAPE), "base": BASE, "K": K, "math": MATH,
         "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls,
         "counts_equal": same,
         "A_ms_rounds": ra, "B_ms_rounds": rb, "A_ms": ma, "B_ms": mb,
         "A_spread_ms": max(ra) - min(ra), "B_minus_A_ms": mb - ma,
         "A_workspace_bytes": plan_a.ws_bytes, "B_workspace_bytes": plan_b.ws_bytes,
         "A_logits_bytes": 4 * K * V,
         "kernels": {
             "k_head_fwd_s": {"ms": t_head, "bytes": by_head, "TBps": rate(by_head, t_head)},
             "spff_confusion": {"ms": t_conf, "bytes": by_conf, "TBps": rate(by_conf, t_conf)},
             "A_head_plus_confusion": {"ms": t_head + t_conf, "bytes": by_head + by_conf,
                                       "TBps": rate(by_head + by_conf, t_head + t_conf)},
             "k_head_mask_s": {"ms": t_mask, "bytes": by_mask, "TBps": rate(by_mask, t_mask),
                               "floor_ms": by_mask / HBM_PEAK * 1e3},
             "k_head_mask_s_with_logits": {"ms": t_mask_lg, "bytes": by_mask_lg,
                                           "TBps": rate(by_mask_lg, t_mask_lg)}}}
    print(json.dumps(r), flush=True)
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "time_predict.json").write_text(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
