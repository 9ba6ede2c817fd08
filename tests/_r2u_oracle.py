"""CPU oracle of the R2UNet3D variant -- TEST INFRASTRUCTURE ONLY.

A functional restatement, in plain PyTorch, of the registry entry "R2UNet3D":
LitR2UNet3D_Published around R2UNet3D_backbone (recurrent residual blocks with
InstanceNorm + ReLU), its replicate pad / centre crop and its foreground-only
soft-Dice loss.  Backward is autograd over this graph.  Works in any dtype
(fp32 to compare with the fixtures, fp64 as the GPU tests' reference) and takes
optional ``relu`` / ``pool`` hooks (tests/_kink.py) so that gradients can be
formed with the ReLU masks / pool argmax of another run.

Pinned to the reference by tests/test_r2unet_cpu.py against
tests/golden/r2u_*.npz (written by tests/golden/make_golden_r2u.py, which runs
the reference's own module).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

BLOCKS = ("e1", "e2", "e3", "e4", "b", "d4", "d3", "d2", "d1")
UPS = ("up4", "up3", "up2", "up1")


@dataclass
class R2UCfg:
    num_classes: int = 13
    base: int = 16
    in_ch: int = 1
    t: int = 2
    pad_multiple: int = 16


def _chans(cfg: R2UCfg):
    f = cfg.base
    cin = [cfg.in_ch, f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f]
    cout = [f, 2 * f, 4 * f, 8 * f, 16 * f, 8 * f, 4 * f, 2 * f, f]
    return cin, cout


def param_shapes(cfg: R2UCfg) -> "OrderedDict[str, Tuple[int, ...]]":
    """Parameters in the Lit module's registration order (backbone.*, head.*)."""
    cin, cout = _chans(cfg)
    f = cfg.base
    out: List[Tuple[str, Tuple[int, ...]]] = []

    def blk(i):
        n, ci, c = "backbone." + BLOCKS[i], cin[i], cout[i]
        return [(n + ".inp.weight", (c, ci, 1, 1, 1)), (n + ".ru.conv.weight", (c, c, 3, 3, 3)),
                (n + ".ru.inn.weight", (c,)), (n + ".ru.inn.bias", (c,)),
                (n + ".out.weight", (c, c, 1, 1, 1)), (n + ".bn.weight", (c,)),
                (n + ".bn.bias", (c,))]
    for i in range(5):
        out += blk(i)
    for u, name in enumerate(UPS):
        out += [(f"backbone.{name}.weight", (16 * f >> u, 8 * f >> u, 2, 2, 2)),
                (f"backbone.{name}.bias", (8 * f >> u,))]
        out += blk(5 + u)
    out += [("head.weight", (cfg.num_classes, f, 1, 1, 1)), ("head.bias", (cfg.num_classes,))]
    return OrderedDict(out)


def params_from_state(state, dtype=torch.float32, requires_grad=True) -> Dict[str, torch.Tensor]:
    return {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(requires_grad)
            for k, v in state.items()}


def _relu(name, r, hooks):
    h = hooks.get("relu") if hooks else None
    return h(name, r) if h else F.relu(r)


def _pool(name, t, hooks):
    h = hooks.get("pool") if hooks else None
    return h(name, t) if h else F.max_pool3d(t, 2)


def _inorm(x, w, b):
    return F.instance_norm(x, None, None, w, b, use_input_stats=True, eps=1e-5)


def _block(P, n, x, t, hooks, saved=None):
    pre = "backbone." + n
    x1 = F.conv3d(x, P[pre + ".inp.weight"])
    h = torch.zeros_like(x1)
    out = x1
    for k in range(1, t + 1):
        z = _inorm(F.conv3d(out + h, P[pre + ".ru.conv.weight"], padding=1),
                   P[pre + ".ru.inn.weight"], P[pre + ".ru.inn.bias"])
        out = _relu(f"{n}.ru{k}", z, hooks)
        h = out
        if saved is not None:
            saved[f"{n}.ru{k}"] = out
    y = F.conv3d(out, P[pre + ".out.weight"])
    o = _relu(f"{n}.out", _inorm(x1 + y, P[pre + ".bn.weight"], P[pre + ".bn.bias"]), hooks)
    if saved is not None:
        saved[f"{n}.x1"] = x1
        saved[f"{n}.out"] = o
    return o


def pad_to_multiple(x, m):
    """Replicate-pad D, H, W up to multiples of m, the odd voxel on the high side."""
    _, _, D, H, W = x.shape
    pd, ph, pw = (-D) % m, (-H) % m, (-W) % m
    if not (pd or ph or pw):
        return x, None
    x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2, pd // 2, pd - pd // 2),
              mode="replicate")
    return x, (D, H, W)


def center_crop(y, orig):
    if orig is None:
        return y
    D, H, W = orig
    _, _, Dn, Hn, Wn = y.shape
    sd, sh, sw = (Dn - D) // 2, (Hn - H) // 2, (Wn - W) // 2
    return y[:, :, sd:sd + D, sh:sh + H, sw:sw + W]


def backbone(P, x, cfg: R2UCfg, hooks=None, saved=None):
    t = cfg.t
    up = lambda v, n: F.conv_transpose3d(v, P[f"backbone.{n}.weight"],  # noqa: E731
                                         P[f"backbone.{n}.bias"], stride=2)
    e1 = _block(P, "e1", x, t, hooks, saved)
    e2 = _block(P, "e2", _pool("pool1", e1, hooks), t, hooks, saved)
    e3 = _block(P, "e3", _pool("pool2", e2, hooks), t, hooks, saved)
    e4 = _block(P, "e4", _pool("pool3", e3, hooks), t, hooks, saved)
    b = _block(P, "b", _pool("pool4", e4, hooks), t, hooks, saved)
    d4 = _block(P, "d4", torch.cat([up(b, "up4"), e4], 1), t, hooks, saved)
    d3 = _block(P, "d3", torch.cat([up(d4, "up3"), e3], 1), t, hooks, saved)
    d2 = _block(P, "d2", torch.cat([up(d3, "up2"), e2], 1), t, hooks, saved)
    return _block(P, "d1", torch.cat([up(d2, "up1"), e1], 1), t, hooks, saved)


def forward(P, x, cfg: R2UCfg, hooks=None, saved=None):
    """Lit forward: pad -> backbone -> 1x1x1 head -> crop."""
    if x.ndim == 4:
        x = x.unsqueeze(1)
    xp, orig = pad_to_multiple(x, cfg.pad_multiple)
    y = F.conv3d(backbone(P, xp, cfg, hooks, saved), P["head.weight"], P["head.bias"])
    return center_crop(y, orig)


def dice_loss(logits, y, ignore_index: Optional[int] = None, eps: float = 1e-6):
    """Foreground-only soft Dice over the samples that have foreground: (loss, dice)."""
    if y.ndim == 5 and y.shape[1] == 1:
        y = y[:, 0]
    K = logits.shape[1]
    p = torch.softmax(logits, dim=1)
    if ignore_index is not None:
        m = (y != ignore_index)
        y = torch.where(m, y, torch.zeros_like(y))
    else:
        m = torch.ones_like(y, dtype=torch.bool)
    mf = m.unsqueeze(1).to(logits.dtype)
    g = F.one_hot(y.long(), K).permute(0, 4, 1, 2, 3).to(logits.dtype) * mf
    p = p * mf
    pf, gf = p[:, 1:], g[:, 1:]
    keep = gf.sum(dim=(1, 2, 3, 4)) > 0
    if K <= 1 or not bool(keep.any()):
        z = logits.sum() * 0.0
        return z, z.detach()
    pf, gf = pf[keep], gf[keep]
    inter = (pf * gf).sum(dim=(2, 3, 4))
    den = (pf + gf).sum(dim=(2, 3, 4))
    dice = ((2 * inter + eps) / (den + eps)).mean()
    return 1.0 - dice, dice.detach()


def fwd_bwd(P, x, labels, cfg: R2UCfg, ignore_index: Optional[int] = 255, hooks=None):
    """One oracle training step with the variant's own loss: (logits, loss, dice)."""
    for t in P.values():
        t.grad = None
    logits = forward(P, x, cfg, hooks)
    loss, dice = dice_loss(logits, labels, ignore_index)
    loss.backward()
    return logits.detach(), loss.detach(), dice
