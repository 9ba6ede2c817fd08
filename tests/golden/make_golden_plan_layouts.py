#!/usr/bin/env python3
"""Record the layout of every engine plan class (tests/golden/plan_layouts.json):

    python tests/golden/make_golden_plan_layouts.py

Creating a plan only computes sizes, so this needs the built library but no GPU.  Per case:
``nfloats``, ``ws_bytes``, the number of parameters and a sha256 over their
``name|shape|off|numel`` lines (UNet3DPlan also ``nbuf`` and its buffer table).  The
workspace offsets themselves are not exported; ``ws_bytes`` is the bump allocator's end, so
it moves when an ``alloc`` is added, dropped or resized, and the parameter digest moves when
a registration does.  tests/test_plan_layouts_cpu.py compares a fresh plan of every case
with the record, which was taken before the plans moved onto the shared PlanBase.
"""
from __future__ import annotations

import hashlib
import json
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / "plan_layouts.json"

# (case id, plan class, constructor arguments); the shapes are those of the CPU tests
_MAIN = dict(batch=1, in_ch=1, depth=5, height=64, width=64, num_classes=13)
_U3D = dict(batch=1, in_ch=1, depth=5, height=32, width=32, target_depth=16)
_SWIN = dict(batch=1, in_ch=1, depth=32, height=32, width=64, num_classes=13)
_UNETR = dict(batch=1, in_ch=1, depth=32, height=32, width=32, num_classes=4, img=(32, 32, 32),
              feature_size=8, hidden=128, mlp_dim=256, heads=2)
_VOL = dict(batch=1, depth=16, height=32, width=32)
CASES = [
    ("plan_registry_k13", "Plan", _MAIN),
    ("plan_registry_k13_f32", "Plan", {**_MAIN, "math": "f32"}),
    ("plan_headline_2x5x128", "Plan", dict(batch=2, in_ch=5, depth=128, height=128, width=128,
                                           num_classes=13)),
    ("plan_512_lean", "Plan", dict(batch=1, in_ch=5, depth=512, height=512, width=512,
                                   num_classes=13)),
    ("plan_height_shard_w4", "Plan", dict(batch=2, in_ch=1, depth=5, height=128, width=512,
                                          num_classes=13, shard_world=4, shard_rank=3,
                                          shard_axis=1)),
    ("unet3d_registry_k13", "UNet3DPlan", {**_U3D, "num_classes": 13, "base": 32}),
    ("unet3d_k40_base24", "UNet3DPlan", {**_U3D, "num_classes": 40, "base": 24}),
    ("unet3d_k40_base24_f32", "UNet3DPlan", {**_U3D, "num_classes": 40, "base": 24,
                                             "math": "f32"}),
    ("swin_smallest", "SwinPlan", _SWIN),
    ("swin_smallest_f32", "SwinPlan", {**_SWIN, "math": "f32"}),
    ("swin_feature4", "SwinPlan", {**_SWIN, "feature_size": 4}),
    ("unetr_ok", "UNETRPlan", _UNETR),
    ("unetr_ok_f32", "UNETRPlan", {**_UNETR, "math": "f32"}),
    ("r2u_base8_t2", "R2UPlan", {**_VOL, "in_ch": 1, "num_classes": 13, "base": 8, "t": 2}),
    ("r2u_base8_t3_f32", "R2UPlan", {**_VOL, "in_ch": 1, "num_classes": 13, "base": 8, "t": 3,
                                     "math": "f32"}),
    ("r2u_base24_t2", "R2UPlan", {**_VOL, "in_ch": 8, "num_classes": 32, "base": 24, "t": 2}),
    ("r2u_base24_t3", "R2UPlan", {**_VOL, "in_ch": 8, "num_classes": 32, "base": 24, "t": 3}),
    ("rupp_base8", "RUPPPlan", {**_VOL, "in_ch": 1, "num_classes": 13, "base": 8}),
    ("rupp_base8_f32", "RUPPPlan", {**_VOL, "in_ch": 1, "num_classes": 13, "base": 8,
                                    "math": "f32"}),
    ("rupp_base24", "RUPPPlan", {**_VOL, "in_ch": 8, "num_classes": 32, "base": 24}),
]


def _digest(lines) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def layout(E, cls: str, kw: dict) -> dict:
    """The recorded quantities of one freshly created plan (E: innovative3D._engine)."""
    plan = getattr(E, cls)(**{"math": "f16x3", **kw})
    rec = {
        "nfloats": plan.nfloats,
        "ws_bytes": plan.ws_bytes,
        "nparams": len(plan.params),
        "params_sha256": _digest(f"{n}|{','.join(map(str, s))}|{o}|{k}"
                                 for n, s, o, k in plan.params),
    }
    if cls == "UNet3DPlan":
        rec["nbuf"] = plan.nbuf
        rec["buffers_sha256"] = _digest(f"{n}|{o}|{k}" for n, o, k in plan.buffers)
    return rec


def main() -> None:
    root = HERE.parents[1]
    sys.path.insert(0, str(root / "spff-unet-spcct_amd"))
    from innovative3D import _engine as E
    OUT.write_text(json.dumps({cid: layout(E, cls, kw) for cid, cls, kw in CASES}, indent=1)
                   + "\n")
    print(f"wrote {OUT} ({len(CASES)} plans)")


if __name__ == "__main__":
    main()
