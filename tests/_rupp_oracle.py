"""CPU oracle of the ResUNet++ variant -- TEST INFRASTRUCTURE ONLY.

A functional restatement, in plain PyTorch, of the registry entry "ResUNet++":
LitResUNetPP3D_Published around ResUNetPP3D_backbone (residual units with InstanceNorm +
ReLU, an ASPP bottleneck of four dilated convs, SE on the encoder outputs, attention gates
at the concats), its replicate pad / centre crop and its batch-pooled soft-Dice + CE loss.
Backward is autograd over this graph.  Works in any dtype (fp32 to compare with the
fixtures, fp64 as the GPU tests' reference) and takes optional ``relu`` / ``pool`` hooks so
that gradients can be formed with the ReLU masks / pool argmax of another run.  ReLU names:
"<unit>.a1", "<unit>.out", "b_aspp.out", "ag<l>.att"; a hook returns None for a name it has
no mask for, and the oracle then uses its own signs.

Pinned to the reference by tests/test_resunetpp_cpu.py against tests/golden/rupp_*.npz
(written by tests/golden/make_golden_rupp.py, which runs the reference's own module).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

UNITS = ("e1", "e2", "e3", "e4", "b_aspp_in", "b_aspp_out", "d4", "d3", "d2", "d1")
LEVEL = dict(zip(UNITS, (0, 1, 2, 3, 4, 4, 3, 2, 1, 0)))
DILATIONS = (1, 2, 4, 8)


@dataclass
class RUPPCfg:
    num_classes: int = 13
    base: int = 16
    in_ch: int = 1
    pad_multiple: int = 16


def param_shapes(cfg: RUPPCfg) -> "OrderedDict[str, Tuple[int, ...]]":
    """Parameters in the Lit module's registration order (backbone.*, head.*)."""
    f = cfg.base
    c = [f, 2 * f, 4 * f, 8 * f, 16 * f]
    out: List[Tuple[str, Tuple[int, ...]]] = []

    def unit(name, ci, co):
        n = "backbone." + name
        r = [(n + ".c1.weight", (co, ci, 3, 3, 3)), (n + ".n1.weight", (co,)), (n + ".n1.bias", (co,)),
             (n + ".c2.weight", (co, co, 3, 3, 3)), (n + ".n2.weight", (co,)), (n + ".n2.bias", (co,))]
        if ci != co:
            r.append((n + ".skip.weight", (co, ci, 1, 1, 1)))
        return r
    out += unit("e1", cfg.in_ch, c[0])
    for i in (1, 2, 3):
        out += unit(f"e{i + 1}", c[i - 1], c[i])
    out += unit("b_aspp_in", c[3], c[4])
    out += [(f"backbone.b_aspp.branches.{r}.weight", (c[4], c[4], 3, 3, 3)) for r in range(4)]
    out += [("backbone.b_aspp.proj.0.weight", (c[4], 4 * c[4], 1, 1, 1))]
    out += unit("b_aspp_out", c[4], c[4])
    for i in range(4):
        h = max(1, c[i] // 16)
        n = f"backbone.se{i + 1}.fc."
        out += [(n + "0.weight", (h, c[i], 1, 1, 1)), (n + "0.bias", (h,)),
                (n + "2.weight", (c[i], h, 1, 1, 1)), (n + "2.bias", (c[i],))]
    for i in (3, 2, 1, 0):
        l = i + 1
        out += [(f"backbone.up{l}.weight", (c[i + 1], c[i], 2, 2, 2)), (f"backbone.up{l}.bias", (c[i],))]
        if i > 0:
            n, I = f"backbone.ag{l}.", c[i] // 2
            out += [(n + "W_x.weight", (I, c[i], 1, 1, 1)), (n + "W_x.bias", (I,)),
                    (n + "W_g.weight", (I, c[i], 1, 1, 1)), (n + "W_g.bias", (I,)),
                    (n + "psi.weight", (1, I, 1, 1, 1)), (n + "psi.bias", (1,))]
        out += unit(f"d{l}", 2 * c[i], c[i])
    out += [("head.weight", (cfg.num_classes, f, 1, 1, 1)), ("head.bias", (cfg.num_classes,))]
    return OrderedDict(out)


def params_from_state(state, dtype=torch.float32, requires_grad=True) -> Dict[str, torch.Tensor]:
    return {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(requires_grad)
            for k, v in state.items()}


def _relu(name, r, hooks):
    h = hooks.get("relu") if hooks else None
    out = h(name, r) if h else None
    return F.relu(r) if out is None else out


def _pool(name, t, hooks):
    h = hooks.get("pool") if hooks else None
    return h(name, t) if h else F.max_pool3d(t, 2)


def _inorm(x, w, b):
    return F.instance_norm(x, None, None, w, b, use_input_stats=True, eps=1e-5)


def _unit(P, n, x, hooks, saved=None):
    pre = "backbone." + n
    s = F.conv3d(x, P[pre + ".skip.weight"]) if pre + ".skip.weight" in P else x
    a1 = _relu(n + ".a1", _inorm(F.conv3d(x, P[pre + ".c1.weight"], padding=1),
                                P[pre + ".n1.weight"], P[pre + ".n1.bias"]), hooks)
    z = _inorm(F.conv3d(a1, P[pre + ".c2.weight"], padding=1), P[pre + ".n2.weight"],
               P[pre + ".n2.bias"])
    o = _relu(n + ".out", z + s, hooks)
    if saved is not None:
        saved[n + ".a1"] = a1
        saved[n + ".out"] = o
    return o


def _aspp(P, x, hooks, saved=None):
    feats = [F.conv3d(x, P[f"backbone.b_aspp.branches.{i}.weight"], padding=d, dilation=d)
             for i, d in enumerate(DILATIONS)]
    o = _relu("b_aspp.out", F.conv3d(torch.cat(feats, 1), P["backbone.b_aspp.proj.0.weight"]), hooks)
    if saved is not None:
        saved["b_aspp.out"] = o
    return o


def _se(P, n, x):
    pre = f"backbone.{n}.fc."
    m = x.mean(dim=(2, 3, 4), keepdim=True)
    h = F.relu(F.conv3d(m, P[pre + "0.weight"], P[pre + "0.bias"]))
    return x * torch.sigmoid(F.conv3d(h, P[pre + "2.weight"], P[pre + "2.bias"]))


def _ag(P, n, x_skip, g, hooks, saved=None):
    """The gate multiplies its first argument (the backbone passes the up-sampled tensor)."""
    pre = f"backbone.{n}."
    att = _relu(n + ".att", F.conv3d(x_skip, P[pre + "W_x.weight"], P[pre + "W_x.bias"]) +
                F.conv3d(g, P[pre + "W_g.weight"], P[pre + "W_g.bias"]), hooks)
    if saved is not None:
        saved[n + ".att"] = att
    return x_skip * torch.sigmoid(F.conv3d(att, P[pre + "psi.weight"], P[pre + "psi.bias"]))


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


def backbone(P, x, cfg: RUPPCfg, hooks=None, saved=None):
    up = lambda v, n: F.conv_transpose3d(v, P[f"backbone.{n}.weight"],  # noqa: E731
                                         P[f"backbone.{n}.bias"], stride=2)
    e1 = _unit(P, "e1", x, hooks, saved)
    e2 = _unit(P, "e2", _pool("pool1", e1, hooks), hooks, saved)
    e3 = _unit(P, "e3", _pool("pool2", e2, hooks), hooks, saved)
    e4 = _unit(P, "e4", _pool("pool3", e3, hooks), hooks, saved)
    b = _unit(P, "b_aspp_in", _pool("pool4", e4, hooks), hooks, saved)
    b = _unit(P, "b_aspp_out", _aspp(P, b, hooks, saved), hooks, saved)
    u4 = up(b, "up4")
    d4 = _unit(P, "d4", torch.cat([u4, _ag(P, "ag4", u4, _se(P, "se4", e4), hooks, saved)], 1),
               hooks, saved)
    u3 = up(d4, "up3")
    d3 = _unit(P, "d3", torch.cat([u3, _ag(P, "ag3", u3, _se(P, "se3", e3), hooks, saved)], 1),
               hooks, saved)
    u2 = up(d3, "up2")
    d2 = _unit(P, "d2", torch.cat([u2, _ag(P, "ag2", u2, _se(P, "se2", e2), hooks, saved)], 1),
               hooks, saved)
    u1 = up(d2, "up1")
    return _unit(P, "d1", torch.cat([u1, _se(P, "se1", e1)], 1), hooks, saved)


def forward(P, x, cfg: RUPPCfg, hooks=None, saved=None):
    """Lit forward: pad -> backbone -> 1x1x1 head -> crop."""
    if x.ndim == 4:
        x = x.unsqueeze(1)
    xp, orig = pad_to_multiple(x, cfg.pad_multiple)
    y = F.conv3d(backbone(P, xp, cfg, hooks, saved), P["head.weight"], P["head.bias"])
    return center_crop(y, orig)


def dice_ce_loss(logits, y, ignore_index: Optional[int] = 255, include_bg: bool = False,
                 ce_weight: float = 1.0, dice_weight: float = 1.0, eps: float = 1e-6):
    """Soft Dice pooled over the whole batch plus the mean CE over valid voxels:
    (loss, mean dice, ce)."""
    K = logits.shape[1]
    p = torch.softmax(logits, dim=1)
    lsm = torch.log_softmax(logits, dim=1)
    if ignore_index is not None:
        m = (y != ignore_index)
        ys = torch.where(m, y, torch.zeros_like(y))
    else:
        m = torch.ones_like(y, dtype=torch.bool)
        ys = y
    mf = m.unsqueeze(1).to(logits.dtype)
    g = F.one_hot(ys.long(), K).permute(0, 4, 1, 2, 3).to(logits.dtype) * mf
    p = p * mf
    dims = (0, 2, 3, 4)
    inter = (p * g).sum(dims)
    den = p.sum(dims) + g.sum(dims)
    dice = (2 * inter + eps) / (den + eps)
    if not include_bg and K > 1:
        dice = dice[1:]
    ce = -(lsm * g).sum() / mf.sum()
    loss = dice_weight * (1.0 - dice.mean()) + ce_weight * ce
    return loss, dice.mean().detach(), ce.detach()


def fwd_bwd(P, x, labels, cfg: RUPPCfg, ignore_index: Optional[int] = 255, hooks=None,
            include_bg: bool = False, ce_weight: float = 0.5, dice_weight: float = 0.5):
    """One oracle training step with the variant's own loss: (logits, loss, dice, ce)."""
    for t in P.values():
        t.grad = None
    logits = forward(P, x, cfg, hooks)
    loss, dice, ce = dice_ce_loss(logits, labels, ignore_index, include_bg, ce_weight, dice_weight)
    loss.backward()
    return logits.detach(), loss.detach(), dice, ce
