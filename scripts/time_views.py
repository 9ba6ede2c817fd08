#!/usr/bin/env python3
"""Time of spff_pred_views (csrc/views.hip), the prediction views of the overlay figures, at
the headline shape 2 x 13 x 128^3 and at the registry's 2 x 13 x 5 x 512^2.

    python scripts/time_views.py [--calls 20] [--warmup 3] [--out DIR]

Synthetic logits N(0, 3^2), channel-last on the device.  Every timed call reads one of four
logits buffers in turn (together > 256 MiB), so no call finds its input in the Infinity
Cache left there by the call before.  Outputs and workspace are allocated once, outside the
events: the call itself allocates nothing and never synchronises.  Each case: warm-up calls,
then >= 20 calls each between two device events on the stream (median, minimum, maximum),
and the same calls back to back between one pair of events (``ms_batched``: launch gaps
overlap).  Per shape, in the same process:

  pred_views        the kernel's own depth split, and forced splits for comparison
  loss_pass         spff_loss (logits read, labels read, dlogits written): the yardstick
                    among the engine's streaming passes
  torch_ops         a restatement in torch device ops (softmax, amax, argmax) on the same
                    tensors
  host_reference    what the reference does for ONE sample: copy its logits to the host and
                    run the per-slice numpy softmax, maxima and argmax there (a numpy
                    restatement of train.py:649-671; one timed run after one warm-up)

``share_of_peak`` is the bytes the pass must move (pred_views: the logits once plus its
outputs; loss_pass: logits + labels + dlogits) over the time, as a share of the HBM peak of
8 TB/s (spec).  There is no pass threshold.

Prints one JSON line per measurement and writes them to DIR/time_views.json (default
bench_out/views).  Needs a ROCm device: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

K = 13
SHAPES = ((2, 128, 128, 128), (2, 5, 512, 512))  # B, D, H, W
HBM_PEAK = 8.0e12  # bytes / s, spec
NBUF = 4


def timed(call, calls, warmup):
    """call(i) enqueues the i-th call.  -> per-call event times and the back-to-back mean"""
    import torch
    for i in range(warmup):
        call(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(calls)]
    for i, (a, b) in enumerate(ev):
        a.record()
        call(i)
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        call(i)
    b.record()
    torch.cuda.synchronize()
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
            "ms_batched": a.elapsed_time(b) / calls}


def rates(r, nbytes):
    r["bytes"] = nbytes
    r["share_of_peak"] = nbytes / (r["ms_median"] * 1e-3) / HBM_PEAK
    r["share_of_peak_batched"] = nbytes / (r["ms_batched"] * 1e-3) / HBM_PEAK
    return r


def host_reference(logits_kdhw):
    """numpy on the host, as train.py:649-671 does it for one sample [K, D, H, W]"""
    import numpy as np

    def soft(L):
        L = L - L.max(axis=0, keepdims=True)
        P = np.exp(L)
        P /= P.sum(axis=0, keepdims=True) + 1e-8
        return P
    D = logits_kdhw.shape[1]
    pc = soft(logits_kdhw[:, D // 2])
    over_d = np.stack([soft(logits_kdhw[:, z]) for z in range(D)], axis=1)
    mip = over_d.max(axis=1)
    return pc.argmax(axis=0), pc.max(axis=0), mip, mip.argmax(axis=0)


def shape_case(B, D, H, W, calls, warmup):
    import ctypes

    import torch
    from innovative3D import _engine as E
    L = E.lib()
    g = torch.Generator(device="cuda").manual_seed(17)
    bufs = [3.0 * torch.randn((B, D, H, W, K), generator=g, device="cuda") for _ in range(NBUF)]
    y = torch.randint(0, K, (B, D, H, W), generator=g, device="cuda")
    n_log = 4 * K * B * D * H * W
    n_out = B * H * W * (1 + 4 + 4 * K + 1)
    base = {"shape": [B, K, D, H, W], "calls": calls, "warmup": warmup,
            "device": torch.cuda.get_device_name(0), "logits_bytes": n_log}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = int(L.spff_pred_views_ws_bytes(B, D, H, W, K))
    ws = torch.empty(max(1, ws_bytes), dtype=torch.uint8, device="cuda")
    cp = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    al = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    mip = torch.empty((B, H, W, K), dtype=torch.float32, device="cuda")
    mp = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    out = []

    def views_call(split):
        def call(i):
            E.check(L.spff_pred_views(E._ptr(bufs[i % NBUF]), B, D, H, W, K, split, E._ptr(cp),
                                      E._ptr(al), E._ptr(mip), E._ptr(mp), E._ptr(ws), stream),
                    "spff_pred_views")
        return call

    for split in (0, 1, 2, 4, 8, 16, 32):
        if split > D:
            continue
        r = rates(timed(views_call(split), calls, warmup), n_log + n_out)
        out.append({**base, "what": "pred_views", "depth_split": split,
                    "workspace_bytes": ws_bytes, **r})
    views_call(0)(0)
    torch.cuda.synchronize()
    got = (cp.clone(), al.clone(), mip.clone(), mp.clone())

    # the loss pass on the same tensors
    out4 = torch.empty(4, dtype=torch.float32, device="cuda")
    dl = torch.empty_like(bufs[0])
    conf = torch.empty(K * (K + 1), dtype=torch.int64, device="cuda")
    lws = E.loss_ws("cuda")
    nvox = B * D * H * W

    def loss_call(i):
        E.check(L.spff_loss(E._ptr(bufs[i % NBUF]), E._ptr(y), nvox, K, 255, 1e-6, None,
                            E._ptr(out4), E._ptr(dl), E._ptr(conf), E._ptr(lws), stream),
                "spff_loss")
    out.append({**base, "what": "loss_pass",
                **rates(timed(loss_call, calls, warmup), 2 * n_log + 8 * nvox)})
    del dl

    # the same views in torch device ops
    keep = {}

    def torch_call(i):
        p = torch.softmax(bufs[i % NBUF], dim=-1)
        pc = p[:, D // 2]
        m = p.amax(dim=1)
        keep["v"] = (pc.argmax(dim=-1), pc.amax(dim=-1), m, m.argmax(dim=-1))
    r = timed(torch_call, calls, warmup)
    torch_call(0)
    torch.cuda.synchronize()
    tv = keep["v"]
    r["center_pred_agree"] = float((tv[0] == got[0]).float().mean())
    r["mip_pred_agree"] = float((tv[3] == got[3]).float().mean())
    r["mip_prob_max_abs_diff"] = float((tv[2] - got[2]).abs().max())
    out.append({**base, "what": "torch_ops", **rates(r, n_log + n_out)})
    keep.clear()

    # the reference's way, one sample: device-to-host copy, then numpy
    one = bufs[0][0].permute(3, 0, 1, 2)  # [K, D, H, W], as the model hands its logits on
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = one.contiguous().cpu().numpy()
        t1 = time.perf_counter()
        hv = host_reference(host)
        t2 = time.perf_counter()
    out.append({**base, "what": "host_reference", "samples": 1, "copy_ms": (t1 - t0) * 1e3,
                "numpy_ms": (t2 - t1) * 1e3, "ms_total": (t2 - t0) * 1e3,
                "center_pred_agree": float((torch.from_numpy(hv[0]).cuda() == got[0][0]).float().mean()),
                "mip_pred_agree": float((torch.from_numpy(hv[3]).cuda() == got[3][0]).float().mean())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "views"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20")
    import torch
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_views: no ROCm device (there is no CPU fallback)")
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []
    for B, D, H, W in SHAPES:
        for r in shape_case(B, D, H, W, a.calls, a.warmup):
            print(json.dumps(r), flush=True)
            lines.append(r)
    (out / "time_views.json").write_text("\n".join(json.dumps(l) for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
