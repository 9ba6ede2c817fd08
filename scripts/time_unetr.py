#!/usr/bin/env python3
"""Step time of the UNETR variant at the registry's training shape.

    python scripts/time_unetr.py [--steps 20] [--warmup 3] [--math f16x3] [--out DIR]

One step = forward + soft-Dice + CE loss + backward of LitUNETR_Published (the registry's
arguments: K 13, img 96^3, feature 16, hidden 768, mlp 3072, 12 heads) on a 1 x 1 x 5 x 512
x 512 input, which the wrapper pads to 16 x 512 x 512, resamples to 96^3 and whose 96^3
logits it resamples back.  Two phases, each a fresh child process under its own time limit
(the second is not started if the first fails or overruns):

  time  warm-up, then >= 20 steps timed with device events, the timer off;
  prof  the same steps with the library-wide timer on (spff_conv_prof_enable): the share
        of the step spent in the 3x3x3 conv kernels per class, in the token path (patch
        embedding, the twelve ViT blocks and the final norm, forward and backward) and in
        the three resampling passes (input, logits, logit gradient).

A kernel trace of one phase alone (no child process; profiles/unetr/kernel_top.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \
        python scripts/time_unetr.py --phase time --steps 20 --warmup 3
    python scripts/kstats.py DIR/.../t_kernel_stats.csv 23 14

Prints one JSON line per phase and writes them to DIR/time_unetr.json (default
bench_out/unetr).  Needs a ROCm device: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "spff-unet-spcct_amd"))

SHAPE = (1, 1, 5, 512, 512)
K, IMG = 13, (96, 96, 96)
LIMIT_S = {"time": 240, "prof": 240}


def _model(math):
    import numpy as np
    import torch
    import innovative3D.models as M
    from innovative3D.weightgen import synth_state
    from innovative3D.config import variant
    m = variant("UNETR")[1]()
    assert isinstance(m, M.LitUNETR_Published) and tuple(m.hparams.img_size) == IMG
    st = synth_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=5)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    m.net.net.math = math
    m = m.to("cuda").train()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(SHAPE, generator=g).to("cuda")
    y = torch.randint(0, K, (SHAPE[0],) + SHAPE[2:], generator=g)
    y[torch.rand(y.shape, generator=g) < 0.03] = 255
    return m, x, y.to("cuda")


def _step(m, x, y):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = m._loss(logits, y)
    loss.backward()
    return loss


def phase(name, steps, warmup, math):
    import torch
    from innovative3D import _engine as E
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("time_unetr: no ROCm device (there is no CPU fallback)")
    m, x, y = _model(math)
    for _ in range(warmup):
        loss = _step(m, x, y)
    torch.cuda.synchronize()
    ws_bytes = m.net.net._plan(torch.empty((1, 1, 16, SHAPE[3], SHAPE[4]), device="cuda")).ws_bytes
    out = {"phase": name, "shape": list(SHAPE), "padded": [16, 512, 512], "K": K, "img": list(IMG),
           "math": math, "steps": steps, "warmup": warmup,
           "device": torch.cuda.get_device_name(0)}
    if name == "prof":
        E.conv_prof_enable(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        loss = _step(m, x, y)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    out["loss"] = float(loss.detach())
    out["workspace_bytes"] = int(ws_bytes)
    out["ms_per_step"] = sum(ms) / steps
    out["ms_min"], out["ms_max"] = min(ms), max(ms)
    if name == "prof":
        prof = E.conv_prof_collect()
        E.conv_prof_enable(False)
        conv_ms = 0.0
        for cls in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
            t_ms, flops, n = prof[cls]
            out[cls] = {"ms_per_step": t_ms / steps, "launches_per_step": n / steps,
                        "tflops": flops / (t_ms * 1e9) if t_ms > 0 else 0.0}
            conv_ms += t_ms / steps
        out["conv_ms_per_step"] = conv_ms
        # (the timer brackets every conv launch with events, which slows the host: the shares
        #  are over THIS phase's step time, the headline ms/step is the other phase's)
        out["conv_share"] = conv_ms / out["ms_per_step"]
        for cls, key in (("unetr_vit", "vit"), ("unetr_resample", "resample")):
            t_ms, _f, n = prof[cls]
            out[key + "_ms_per_step"] = t_ms / steps
            out[key + "_brackets_per_step"] = n / steps
            out[key + "_share"] = t_ms / steps / out["ms_per_step"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--math", default="f16x3")
    ap.add_argument("--out", default=str(ROOT / "bench_out" / "unetr"))
    ap.add_argument("--phase", choices=("time", "prof"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be >= 20")
    if a.phase:
        phase(a.phase, a.steps, a.warmup, a.math)
        return 0
    out = pathlib.Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    lines = []
    for name in ("time", "prof"):
        cmd = [sys.executable, __file__, "--phase", name, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--math", a.math]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[name])
        except subprocess.TimeoutExpired:
            print(f"time_unetr: phase {name} exceeded {LIMIT_S[name]} s; stopping", file=sys.stderr)
            return 124
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:
            print(f"time_unetr: phase {name} failed ({r.returncode}); stopping", file=sys.stderr)
            return r.returncode or 1
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    (out / "time_unetr.json").write_text("\n".join(json.dumps(l) for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
