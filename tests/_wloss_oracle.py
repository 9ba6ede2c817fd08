"""CPU oracle of the two losses of csrc/soft_dice.hip's DICE_UNET3D and DICE_NNUNET kinds --
TEST INFRASTRUCTURE ONLY.

Plain PyTorch in any dtype (fp32 to compare with the fixtures, fp64 as the GPU tests'
reference), with the closed-form dlogits the gradient pass implements next to each loss, so
that the closed forms can be checked against autograd of the same loss.

  unet3d_loss   LitCicek3DUNet_DepthAdapter_Published._weighted_softmax_ce + ._dice_loss
  nnunet_loss   models.dice_ce_loss (soft_dice_loss_from_logits + cross_entropy)

Both define what the reference cannot express: a label outside [0, K) that is not
ignore_index counts as ignored (mask 0, no term in any sum, a zero dlogits row).

Pinned to the reference by tests/test_weighted_loss_cpu.py against
tests/golden/unet3d_loss_small.npz and nnunet_loss_small.npz (written by
tests/golden/make_golden_wloss.py, which runs the reference's own functions).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F


def fixture_case(z, c, weights=False):
    """Case ``c`` of a loaded *_loss_small.npz: (logits, labels, keyword arguments of the
    oracle's functions); ``weights``: with the 3DUNet fixture's class / voxel weights (None
    where the case has none)."""
    kw = dict(ignore_index=int(z[f"{c}/ignore"]) if int(z[f"{c}/use_ignore"]) else None,
              include_bg=bool(int(z[f"{c}/include_bg"])), ce_weight=float(z[f"{c}/ce_weight"]),
              dice_weight=float(z[f"{c}/dice_weight"]))
    if weights:
        for k in ("class_weights", "voxel_weights"):
            kw[k] = torch.from_numpy(z[f"{c}/{k}"]) if f"{c}/{k}" in z.files else None
    return torch.from_numpy(z[f"{c}/logits"]), torch.from_numpy(z[f"{c}/labels"]), kw


def _parts(logits, y, ignore_index):
    """(m [B,1,...], g [B,K,...] one-hot of the unmasked labels, p = softmax, log p)"""
    K = logits.shape[1]
    m = (y >= 0) & (y < K)
    if ignore_index is not None:
        m = m & (y != ignore_index)
    ys = torch.where(m, y, torch.zeros_like(y))
    mf = m.unsqueeze(1).to(logits.dtype)
    g = F.one_hot(ys.long(), K).movedim(-1, 1).to(logits.dtype) * mf
    return mf, g, torch.softmax(logits, dim=1), torch.log_softmax(logits, dim=1)


def _sum_sp(t):
    return t.flatten(2).sum(-1)  # [B, K]


def _softmax_vjp(p, gam):
    """dlogits of a loss with dL/dp = gam: p (gam - <p, gam>)"""
    return p * (gam - (p * gam).sum(1, keepdim=True))


def unet3d_loss(logits, y, ignore_index: Optional[int] = 255, class_weights=None,
                voxel_weights=None, include_bg: bool = False, ce_weight: float = 1.0,
                dice_weight: float = 0.0, eps: float = 1e-6):
    """-> (loss, ce, dice_loss, sum m u); loss = ce_weight ce + dice_weight dice_loss with
    ce = sum m u w[y] nll / max(sum m u, 1) and dice_loss = 1 - mean_{b, k >= sc} 2 I /
    (P + G + eps), the sums per sample."""
    dt = logits.dtype
    K = logits.shape[1]
    mf, g, p, lsm = _parts(logits, y, ignore_index)
    u = torch.ones_like(mf) if voxel_weights is None else \
        torch.as_tensor(voxel_weights).to(dt).reshape(mf.shape)
    w = torch.ones(K, dtype=dt) if class_weights is None else torch.as_tensor(class_weights).to(dt)
    wy = (g * w.view(1, K, *([1] * (logits.ndim - 2)))).sum(1, keepdim=True)  # m w[y]
    nll = -(lsm * g).sum(1, keepdim=True)                                      # m nll
    usum = (mf * u).sum()
    ce = (wy * nll * u).sum() / usum.clamp_min(1.0)
    sc = 0 if include_bg else 1
    pm = p * mf
    inter, den = _sum_sp(pm * g), _sum_sp(pm) + _sum_sp(g) + eps
    dice_loss = 1.0 - (2.0 * inter / den)[:, sc:].mean()
    return ce_weight * ce + dice_weight * dice_loss, ce, dice_loss, usum


def unet3d_dlogits(logits, y, ignore_index: Optional[int] = 255, class_weights=None,
                   voxel_weights=None, include_bg: bool = False, ce_weight: float = 1.0,
                   dice_weight: float = 0.0, eps: float = 1e-6):
    """The closed form: p (Gam - <p, Gam>) + c (p - g), Gam_k = m (alpha_bk g_k + beta_bk),
    alpha = -2 dw / (B nc den), beta = 2 dw I / (B nc den^2), c = cw m u w[y] / max(sum m u, 1)."""
    dt = logits.dtype
    B, K = logits.shape[:2]
    sp = [1] * (logits.ndim - 2)
    mf, g, p, _lsm = _parts(logits, y, ignore_index)
    u = torch.ones_like(mf) if voxel_weights is None else \
        torch.as_tensor(voxel_weights).to(dt).reshape(mf.shape)
    w = torch.ones(K, dtype=dt) if class_weights is None else torch.as_tensor(class_weights).to(dt)
    wy = (g * w.view(1, K, *sp)).sum(1, keepdim=True)
    sc = 0 if include_bg else 1
    nc = K - sc
    pm = p * mf
    inter, den = _sum_sp(pm * g), _sum_sp(pm) + _sum_sp(g) + eps
    alpha = -2.0 * dice_weight / (B * nc * den)
    beta = 2.0 * dice_weight * inter / (B * nc * den * den)
    alpha[:, :sc] = 0
    beta[:, :sc] = 0
    gam = mf * (alpha.view(B, K, *sp) * g + beta.view(B, K, *sp))
    c = ce_weight * wy * u / (mf * u).sum().clamp_min(1.0)
    return _softmax_vjp(p, gam) + c * (p * mf - g)


def nnunet_loss(logits, y, ignore_index: Optional[int] = -1, include_bg: bool = False,
                ce_weight: float = 1.0, dice_weight: float = 1.0, eps: float = 1e-5):
    """-> (loss, ce, dice_mean, N_valid); loss = ce_weight CE + dice_weight (1 - mean_{k >= sc}
    (2 I_k + eps) / (Q_k + G_k + eps)), I, Q = sum m p^2 and G pooled over the batch."""
    mf, g, p, lsm = _parts(logits, y, ignore_index)
    sc = 0 if include_bg else 1
    pm = p * mf
    inter = _sum_sp(pm * g).sum(0)
    den = _sum_sp(pm * pm).sum(0) + _sum_sp(g).sum(0) + eps
    dice = ((2.0 * inter + eps) / den)[sc:].mean()
    n = mf.sum()
    ce = -(lsm * g).sum() / n  # 0 / 0 -> nan, as F.cross_entropy
    return ce_weight * ce + dice_weight * (1.0 - dice), ce, dice, n


def nnunet_dlogits(logits, y, ignore_index: Optional[int] = -1, include_bg: bool = False,
                   ce_weight: float = 1.0, dice_weight: float = 1.0, eps: float = 1e-5):
    """The closed form: p (Gam - <p, Gam>) + (cw / N)(p - g), Gam_k = m (alpha_k g_k + gamma_k
    p_k), alpha = -2 dw / (nc den), gamma = 2 dw (2 I + eps) / (nc den^2)."""
    K = logits.shape[1]
    sp = [1] * (logits.ndim - 2)
    mf, g, p, _lsm = _parts(logits, y, ignore_index)
    sc = 0 if include_bg else 1
    nc = K - sc
    pm = p * mf
    inter = _sum_sp(pm * g).sum(0)
    den = _sum_sp(pm * pm).sum(0) + _sum_sp(g).sum(0) + eps
    alpha = -2.0 * dice_weight / (nc * den)
    gamma = 2.0 * dice_weight * (2.0 * inter + eps) / (nc * den * den)
    alpha[:sc] = 0
    gamma[:sc] = 0
    gam = mf * (alpha.view(1, K, *sp) * g + gamma.view(1, K, *sp) * p)
    return _softmax_vjp(p, gam) + (ce_weight / mf.sum()) * (p * mf - g)
