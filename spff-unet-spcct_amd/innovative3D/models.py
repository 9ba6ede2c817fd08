"""SPFF-UNet model family -- drop-in mirror of innovative3D/models.py whose
forward/backward run on the MI355X HIP engine (libspff_hip.so).

The module tree (names, parameter shapes, registration order, the lazily
created and aliased FourierGate mask) is identical to the reference, so
state_dicts / checkpoints move between the two unchanged.  The nn.Conv3d /
nn.InstanceNorm3d / ... children are parameter containers only: their
forward is never called.  ``UNet3D_SpectralCore.forward`` hands the input and
one flat fp32 parameter buffer (the Parameters are views into it) to the
engine through a torch.autograd.Function; autograd receives the engine's
flat gradient back as per-parameter views.

Reference map (models.py): _SEChannelLite 600-609, _SpectralSE 611-614,
_conv3x3xk 616-618, _DoubleConvSpectral 620-625, UNet3D_SpectralCore 647-701,
_LitSPCT_Base 703-712, upgrade_spct_with_novel_blocks 1416-1446,
_DoubleConvSpectral_Novel 1448-1478, EnergyFiLM3D 1479-1512, FourierGate3D
1515-1544, build_spct_energyfilm_fourier 1547-1555, LitSPCT_* 1558-1607,
BaseLitModel 466-594.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _engine as E
from .config import BEST_LR, IGNORE_INDEX, NUM_CLASSES, NUM_FRAMES  # noqa: F401
from .helpers import (LOSS_REGISTRY, _DeviceLoss, _logits_cl, ce_plus_macro_dice_loss,  # noqa: F401
                      ce_dice_with_confusion, fast_simple_metrics, metrics_from_confusion,
                      per_class_metrics_2d, per_class_metrics_3d, ranking_metrics)
from .helpers import predict_tiled as _predict_tiled
from .lightning_compat import pl

# ----------------------------------------------------------------- utilities --


def _pick_first_if_seq(x):
    return x[0] if isinstance(x, (list, tuple)) else x


def _image_label(batch):
    """(image, label) of an (x, y) pair or an {"image", "label"} dict batch"""
    return batch if isinstance(batch, (list, tuple)) else (batch["image"], batch["label"])


def _canonicalize_targets_2d(lbls):
    lbls = _pick_first_if_seq(lbls)
    if not torch.is_tensor(lbls):
        lbls = torch.as_tensor(lbls)
    if lbls.ndim == 4:
        lbls = lbls.max(dim=1).values
    elif lbls.ndim == 2:
        lbls = lbls.unsqueeze(0)
    return lbls.long()


def _canonicalize_targets_3d(lbls):
    """(B,1,F,H,W)/(B,F,H,W,1)/(F,H,W) -> (B,F,H,W) long (models.py:69-84)."""
    lbls = _pick_first_if_seq(lbls)
    if not torch.is_tensor(lbls):
        lbls = torch.as_tensor(lbls)
    if lbls.ndim == 5 and lbls.size(1) == 1:
        lbls = lbls[:, 0]
    if lbls.ndim == 5 and lbls.size(-1) == 1:
        lbls = lbls[..., 0]
    if lbls.ndim == 3:
        lbls = lbls.unsqueeze(0)
    assert lbls.ndim == 4, f"Need (B,F,H,W) labels, got {tuple(lbls.shape)}"
    return lbls.long()


def _next_mult(n: int, m: int = 16) -> int:
    return ((n + m - 1) // m) * m


def _pad_to_mult_3d(x: torch.Tensor, m: int = 16):
    """Replicate-pad D/H/W to multiples of m (models.py:109-120)."""
    B, C, D, H, W = x.shape
    Dn, Hn, Wn = _next_mult(D, m), _next_mult(H, m), _next_mult(W, m)
    pd, ph, pw = Dn - D, Hn - H, Wn - W
    if not (pd or ph or pw):
        return x, None
    x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2, pd // 2, pd - pd // 2),
              mode="replicate")
    return x, (D, H, W)


def _center_crop_to_3d(x: torch.Tensor, orig_dhw):
    if orig_dhw is None:
        return x
    D, H, W = orig_dhw
    _, _, Dn, Hn, Wn = x.shape
    sd, sh, sw = (Dn - D) // 2, (Hn - H) // 2, (Wn - W) // 2
    return x[:, :, sd:sd + D, sh:sh + H, sw:sw + W]


_center_crop_3d = _center_crop_to_3d


# ------------------------------------------- nnU-Net style Dice + CE loss --
class _NNUNetLoss(_DeviceLoss):
    """(logits, labels, K, ignore_index, include_bg, ce_weight, dice_weight) ->
    (loss, out4 = [ce, loss, dice_mean, N_valid]); only the loss carries a gradient."""

    WHAT = "nnU-Net Dice+CE loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl = E.nnunet_loss_forward(lcl, labels, *args)
        return dl, out4[1].clone(), out4


def _nnunet_loss(logits, labels, num_classes, ignore_index, include_background, ce_weight,
                 dice_weight, eps=1e-5):
    if eps != 1e-5:
        raise NotImplementedError("the loss kernel's eps is 1e-5")
    if logits.ndim != 5 or labels.ndim != 4:
        raise ValueError(f"expected [B,K,D,H,W] logits and [B,D,H,W] labels, got "
                         f"{tuple(logits.shape)} and {tuple(labels.shape)}")
    if int(num_classes) != logits.shape[1]:
        raise ValueError(f"num_classes {num_classes} != logits' {logits.shape[1]} channels")
    return _NNUNetLoss.apply(logits, labels, int(num_classes), int(ignore_index),
                             bool(include_background), float(ce_weight), float(dice_weight))[0]


def soft_dice_loss_from_logits(logits: torch.Tensor, labels: torch.Tensor, num_classes: int,
                               ignore_index: int = -1, include_background: bool = False,
                               eps: float = 1e-5) -> torch.Tensor:
    """models.py:254-275: 1 - mean_k (2 I_k + eps) / (sum m p_k^2 + sum m g_k + eps), the sums
    pooled over the batch.  The HIP loss driver with ce_weight 0."""
    return _nnunet_loss(logits, labels, num_classes, ignore_index, include_background, 0.0, 1.0,
                        eps)


def dice_ce_loss(logits: torch.Tensor, labels: torch.Tensor, num_classes: int,
                 ignore_index: int = -1, ce_weight: float = 1.0, dice_weight: float = 1.0,
                 include_background: bool = False) -> torch.Tensor:
    """models.py:277-290: ce_weight * cross_entropy + dice_weight * soft_dice_loss_from_logits,
    one call of the HIP loss driver."""
    return _nnunet_loss(logits, labels, num_classes, ignore_index, include_background, ce_weight,
                        dice_weight)


def _norm3d(c: int, kind: str = "instance") -> nn.Module:
    if not (kind or "instance").lower().startswith("inst"):
        raise NotImplementedError("SPFF engine implements InstanceNorm3d(affine) only "
                                  "(models.py:168-173; SPFF never selects another norm)")
    return nn.InstanceNorm3d(c, affine=True, eps=1e-5)


def _act(kind: str = "lrelu") -> nn.Module:
    if not (kind or "lrelu").lower().startswith("lrel"):
        raise NotImplementedError("SPFF engine implements LeakyReLU(0.01) only (models.py:175-181)")
    return nn.LeakyReLU(1e-2, inplace=True)


def _conv3x3xk(cin, cout, ksd=1, bias=False):
    return nn.Conv3d(cin, cout, kernel_size=(ksd, 3, 3), padding=(ksd // 2, 1, 1), bias=bias)


# ------------------------------------------------------- parameter containers --
class _SEChannelLite(nn.Module):
    def __init__(self, c, r=16):
        super().__init__()
        h = max(4, c // r)
        self.pool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Sequential(nn.Conv3d(c, h, 1, bias=True), nn.ReLU(inplace=True),
                                nn.Conv3d(h, c, 1, bias=True), nn.Sigmoid())


class _SpectralSE(nn.Module):
    pass


class SpatialAttention3D(nn.Module):
    """CBAM-style spatial attention (models.py:434-446): parameter container; the engine
    runs mean / max over the channels, the 2 -> 1 channel stencil, the sigmoid and the
    product."""

    def __init__(self, kernel_size=(3, 7, 7)):
        super().__init__()
        if tuple(kernel_size) != (3, 7, 7):
            raise NotImplementedError("SpatialAttention3D: the engine's stencil is (3, 7, 7)")
        self.conv = nn.Conv3d(2, 1, kernel_size=(3, 7, 7), padding=(1, 3, 3), bias=False)
        self.sigmoid = nn.Sigmoid()


class AttentionGate(nn.Module):
    """3D attention gate for skip connections (models.py:627-640): parameter container.
    forward(x_skip, g) = x_skip * sigmoid(psi(relu(W_x x_skip + W_g g))): the gate multiplies
    its first argument."""

    def __init__(self, F_skip, F_g, F_int=None):
        super().__init__()
        if F_int is None:
            F_int = min(F_skip, F_g)
        self.W_x = nn.Conv3d(F_skip, F_int, 1, 1, 0, bias=True)
        self.W_g = nn.Conv3d(F_g, F_int, 1, 1, 0, bias=True)
        self.psi = nn.Conv3d(F_int, 1, 1, 1, 0, bias=True)
        nn.init.constant_(self.psi.bias, 0.0)
        self.relu = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()


class _DoubleConvSpectral(nn.Module):
    def __init__(self, cin, cout, ksd=1, norm="instance", act="lrelu"):
        super().__init__()
        self.b1 = nn.Sequential(_conv3x3xk(cin, cout, ksd, bias=False), _norm3d(cout, norm), _act(act))
        self.b2 = nn.Sequential(_conv3x3xk(cout, cout, ksd, bias=False), _norm3d(cout, norm), _act(act))


class EnergyFiLM3D(nn.Module):
    """models.py:1479-1512 (parameter container; the engine computes it).  hidden 1..64,
    pe_dims 2..32 (include/spff.h spff_cfg.efilm_hidden / efilm_pe_dims), the same in every
    block of a network."""

    def __init__(self, channels: int, hidden: int = 32, pe_dims: int = 16):
        super().__init__()
        if not (1 <= int(hidden) <= 64 and 2 <= int(pe_dims) <= 32):
            raise NotImplementedError(
                f"EnergyFiLM3D(hidden={hidden}, pe_dims={pe_dims}): the engine supports hidden "
                "1..64 and pe_dims 2..32 (reference models.py:1484; pe_dims 1 makes the "
                "reference's own Conv1d raise); see INTEGRATION.md §2")
        self.channels = int(channels)
        self.hidden = int(hidden)
        self.pe_dims = int(pe_dims)
        self.mlp = nn.Sequential(nn.Conv1d(self.pe_dims, hidden, 1, bias=True), nn.ReLU(inplace=True),
                                 nn.Conv1d(hidden, 2 * self.channels, 1, bias=True))


class FourierGate3D(nn.Module):
    """Same lazy mask semantics as the reference (models.py:1527-1535):
    ``_mask``/``freq_mask`` (one tensor, two names) appear at the first forward.
    learn_phase=True multiplies the spectrum by (M + 0.01 i) (models.py:1538-1539), on the
    engine as an extra real circulant term (gates.hip phase_term)."""

    def __init__(self, learn_phase: bool = False):
        super().__init__()
        self.learn_phase = bool(learn_phase)
        self.mag_scale = nn.Parameter(torch.ones(1))
        self._mask = None

    def _ensure_mask(self, Fdim: int, device):
        L = Fdim // 2 + 1
        if (self._mask is None) or (self._mask.shape[2] != L):
            self._mask = nn.Parameter(torch.ones(1, 1, L, 1, 1, device=device,
                                                 dtype=self.mag_scale.dtype))
            self.register_parameter("freq_mask", self._mask)


class _DoubleConvSpectral_Novel(nn.Module):
    def __init__(self, cin, cout, ksd=1, norm="instance", act="lrelu", use_efilm: bool = False,
                 use_fouriergate: bool = False, use_moe: bool = False, moe_K: int = 3):
        super().__init__()
        if use_moe:
            # SpectralMoE3D is referenced but never defined in the reference (models.py:1464)
            raise NotImplementedError("use_moe: SpectralMoE3D does not exist in the reference")
        self.pre = nn.Sequential(_conv3x3xk(cin, cout, ksd, bias=False), _norm3d(cout, norm), _act(act))
        self.body = nn.Sequential(_conv3x3xk(cout, cout, ksd, bias=False), _norm3d(cout, norm), _act(act))
        self.efilm = EnergyFiLM3D(cout) if use_efilm else nn.Identity()
        self.fgate = FourierGate3D() if use_fouriergate else nn.Identity()


# --------------------------------------------------------- engine autograd op --
def _mark_covered(grad_hook, param_ids) -> None:
    """tell a GradBucketer which parameters' gradients it all-reduced (their flat
    gradient went through its buckets), so the caller reduces only the rest"""
    if grad_hook is not None and hasattr(grad_hook, "cover"):
        grad_hook.cover(param_ids)


class _PlanFunction(torch.autograd.Function):
    """One forward / backward of an engine plan (any E._PlanBase) as an autograd node.
    ``extra``: the plan's own forward arguments after ``flat`` -- (bufs, training) for the
    3DUNet, () otherwise."""

    @staticmethod
    def forward(ctx, x, plan, flat, grad_hook, extra, *params):
        logits_cl = plan.forward(x, flat, *extra)
        ctx.plan, ctx.gen, ctx.flat, ctx.grad_hook = plan, plan.generation, flat, grad_hook
        # a backward is pending on this workspace (E._alloc_workspace releases other
        # plans' workspaces on OOM, pending ones only as a last resort)
        plan._pending_gen = plan.generation if any(ctx.needs_input_grad) else None
        ctx.param_ids = tuple(id(p) for p in params)
        ctx.slices = [(off, n, shape) for (_name, shape, off, n) in plan.params]
        return logits_cl.permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        if plan.generation != ctx.gen:
            if isinstance(plan, E.Plan):
                raise E.SpffError("SPFF engine: another forward ran on this model (or its cached "
                                  "workspace was released for another plan's) before the backward "
                                  "of this one; the engine keeps one forward's activations per model")
            raise E.SpffError(f"{plan.NAME} engine: another forward ran on this model before the "
                              "backward of this one; the engine keeps one forward's activations")
        g_cl = g.permute(0, 2, 3, 4, 1).contiguous()
        dflat = plan.backward(g_cl, ctx.flat, grad_hook=ctx.grad_hook)
        plan._pending_gen = None
        _mark_covered(ctx.grad_hook, ctx.param_ids)
        grads = [dflat[o:o + n].view(s) for (o, n, s) in ctx.slices]
        return (None, None, None, None, None, *grads)


class _FlatParamMixin:
    """For a module whose Parameters are views into its plan's one flat fp32 buffer, under
    the plan's parameter names: every engine-backed module here."""

    _DUPLICATE_PARAMS = False  # True: tied parameters keep every name they are registered under

    def _engine_params(self, plan) -> List[nn.Parameter]:
        named = dict(self.named_parameters(remove_duplicate=not self._DUPLICATE_PARAMS))
        out = []
        for name, shape, _off, _n in plan.params:
            p = named.get(name)
            if p is None or tuple(p.shape) != tuple(shape):
                raise E.SpffError(f"parameter {name} {shape} missing or mis-shaped in the module")
            out.append(p)
        return out

    def _ensure_flat(self, plan, params, device) -> torch.Tensor:
        flat = self._flat
        ok = flat is not None and flat.device == device and flat.numel() == plan.nfloats
        if ok:
            base = flat.data_ptr()
            ok = all(p.data_ptr() == base + 4 * off and p.dtype == torch.float32
                     for p, (_n, _s, off, _k) in zip(params, plan.params))
        if not ok:
            flat = torch.empty(plan.nfloats, dtype=torch.float32, device=device)
            with torch.no_grad():
                for p, (_name, shape, off, n) in zip(params, plan.params):
                    flat[off:off + n].copy_(p.detach().reshape(-1).to(device=device,
                                                                     dtype=torch.float32))
                    p.data = flat[off:off + n].view(shape)
            self._flat = flat
        return flat

    def _run_plan(self, plan, x, extra=()):
        """x [B,Cin,D,H,W] -> logits [B,K,D,H,W] of ``plan`` on this module's parameters,
        through autograd when a gradient is wanted (``extra``: see _PlanFunction)."""
        params = self._engine_params(plan)
        flat = self._ensure_flat(plan, params, x.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _PlanFunction.apply(x.float(), plan, flat, getattr(self, "grad_hook", None),
                                       extra, *params)
        return plan.forward(x.float(), flat, *extra).permute(0, 4, 1, 2, 3)


# -------------------------------------------------------------------- core ----
class UNet3D_SpectralCore(_FlatParamMixin, nn.Module):
    """Depth-preserving 3-level UNet (models.py:647-701).  forward runs on the
    HIP engine; pool/upsample act in (H,W) only, so D is arbitrary while H, W
    must be multiples of 8."""

    _DUPLICATE_PARAMS = True

    def __init__(self, in_channels=1, num_classes=2, base=32, ksd=3, use_se=False,
                 use_specse=False, use_spatial=False, use_skip_gate=False, norm="instance",
                 act="lrelu"):
        super().__init__()
        f = int(base)
        P = (1, 2, 2)
        self.in_channels, self.num_classes, self.base, self.ksd = int(in_channels), int(num_classes), f, int(ksd)
        self.use_se, self.use_specse = bool(use_se), bool(use_specse)
        self.use_spatial, self.use_skip_gate = bool(use_spatial), bool(use_skip_gate)
        self.enc1 = _DoubleConvSpectral(in_channels, f, ksd, norm, act)
        self.pool1 = nn.MaxPool3d(P)
        self.enc2 = _DoubleConvSpectral(f, 2 * f, ksd, norm, act)
        self.pool2 = nn.MaxPool3d(P)
        self.enc3 = _DoubleConvSpectral(2 * f, 4 * f, ksd, norm, act)
        self.pool3 = nn.MaxPool3d(P)
        self.bott = _DoubleConvSpectral(4 * f, 8 * f, ksd, norm, act)
        self.up3 = nn.ConvTranspose3d(8 * f, 4 * f, kernel_size=P, stride=P)
        self.dec3 = _DoubleConvSpectral(8 * f, 4 * f, ksd, norm, act)
        self.up2 = nn.ConvTranspose3d(4 * f, 2 * f, kernel_size=P, stride=P)
        self.dec2 = _DoubleConvSpectral(4 * f, 2 * f, ksd, norm, act)
        self.up1 = nn.ConvTranspose3d(2 * f, f, kernel_size=P, stride=P)
        self.dec1 = _DoubleConvSpectral(2 * f, f, ksd, norm, act)
        self.out = nn.Conv3d(f, num_classes, 1)
        self.se = nn.ModuleList([_SEChannelLite(c) if use_se else nn.Identity() for c in (f, 2 * f, 4 * f, 8 * f)])
        self.sp = nn.ModuleList([_SpectralSE() if use_specse else nn.Identity() for _ in range(4)])
        self.sa = nn.ModuleList([SpatialAttention3D() if use_spatial else nn.Identity()
                                 for _ in range(4)])
        # gated skips: the SPCT core's gates are the base AttentionGate called as
        # (g_c, x_c, inter_c) -> (F_skip = x_c, F_g = g_c, F_int) (models.py:642-645)
        self.g3 = AttentionGate(4 * f, 4 * f, 2 * f) if use_skip_gate else None
        self.g2 = AttentionGate(2 * f, 2 * f, f) if use_skip_gate else None
        self.g1 = AttentionGate(f, f, f // 2) if use_skip_gate else None
        self._plan = None
        self._flat = None
        self._infer_plan = None

    # ---- flags derived from the (possibly upgraded) module tree ----
    def _blocks(self):
        return [self.enc1, self.enc2, self.enc3, self.bott, self.dec3, self.dec2, self.dec1]

    def _flags(self) -> Tuple[bool, bool]:
        kinds = set()
        for b in self._blocks():
            if isinstance(b, _DoubleConvSpectral_Novel):
                kinds.add((isinstance(b.efilm, EnergyFiLM3D), isinstance(b.fgate, FourierGate3D)))
            else:
                kinds.add((False, False))
        if len(kinds) != 1:
            raise NotImplementedError("mixed block kinds; upgrade_spct_with_novel_blocks upgrades all")
        return next(iter(kinds))

    def _gate_settings(self) -> dict:
        """EnergyFiLM3D(hidden, pe_dims) / FourierGate3D(learn_phase) of the blocks (one
        setting for the whole network: include/spff.h spff_cfg)"""
        ef = {(b.efilm.hidden, b.efilm.pe_dims) for b in self._blocks()
              if isinstance(getattr(b, "efilm", None), EnergyFiLM3D)}
        ph = {b.fgate.learn_phase for b in self._blocks()
              if isinstance(getattr(b, "fgate", None), FourierGate3D)}
        if len(ef) > 1 or len(ph) > 1:
            raise NotImplementedError("EnergyFiLM3D(hidden, pe_dims) / FourierGate3D(learn_phase) "
                                      "must be the same in every block on the engine")
        h, pdim = next(iter(ef)) if ef else (32, 16)
        return {"efilm_hidden": h, "efilm_pe_dims": pdim,
                "fgate_learn_phase": bool(next(iter(ph))) if ph else False}

    def _engine_plan(self, x: torch.Tensor, tag: str, memory: Optional[str] = None):
        """``memory``: the layout of this plan instead of the module's ``.memory``"""
        memory = memory or getattr(self, "memory", None)
        B, C, D, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"expected {self.in_channels} input channels, got {C}")
        efilm, fgate = self._flags()
        # sharding (innovative3D.sharded): x is this rank's D-slab of a volume of
        # depth D * world (axis 0), or its H-slab of a volume of height H * world
        # (axis 1, the registry layout); the FourierGate acts on the full depth
        shard = E.shard_key(getattr(self, "shard", (1, 0)))
        if self.use_spatial or self.use_skip_gate:  # before any device call
            if shard[0] > 1:
                raise E.SpffError("use_spatial / use_skip_gate run on unsharded modules only: the "
                                  "3x7x7 stencil needs halos the shard collectives do not carry")
            if memory in ("lean", "infer"):
                raise E.SpffError("use_spatial / use_skip_gate: the lean layout does not "
                                  "recompute them and the forward-only one does not place "
                                  "them; use memory 'full' or 'auto'")
            if self.use_skip_gate and (H % 8 or W % 8):
                raise E.SpffError("use_skip_gate needs H and W multiples of 8: the reference's "
                                  "gate fails where an up-conv output and its skip differ")
        if fgate:
            for b in self._blocks():
                b.fgate._ensure_mask(D * (shard[0] if shard[2] == 0 else 1), x.device)
        plan = E.get_plan(batch=B, in_ch=C, depth=D, height=H, width=W,
                          num_classes=self.num_classes, base=self.base, ksd=self.ksd,
                          efilm=efilm, fgate=fgate, se=self.use_se, specse=self.use_specse,
                          device=x.device, math=getattr(self, "math", None), shard=shard,
                          memory=memory, spatial=self.use_spatial,
                          skip_gate=self.use_skip_gate,
                          owner=self, tag=tag, **self._gate_settings())
        if shard[0] > 1:
            coll = getattr(self, "shard_coll", None)
            if coll is None:
                raise E.SpffError("sharded module: set .shard_coll (innovative3D.sharded)")
            if getattr(plan, "coll_impl", None) is not coll:
                plan.set_coll(coll)
        return plan

    def forward(self, x):
        x = _pick_first_if_seq(x)
        E.require_device(x, "UNet3D_SpectralCore.forward")
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad and getattr(self, "memory", None) == "infer":
            raise E.SpffError("memory = 'infer' is the forward-only layout: run the forward "
                              "under torch.no_grad(), or leave .memory unset to train")
        plan = self._engine_plan(x, "train" if need_grad else "infer")
        params = self._engine_params(plan)
        flat = self._ensure_flat(plan, params, x.device)
        if need_grad:
            self._plan = plan
            return _PlanFunction.apply(x.float(), plan, flat, getattr(self, "grad_hook", None), (),
                                       *params)
        self._infer_plan = plan
        logits_cl = plan.forward(x.float(), flat)
        return logits_cl.permute(0, 4, 1, 2, 3)

    @torch.no_grad()
    def predict(self, x, labels=None, ignore_index=None, return_logits=False):
        """The segmentation of x on a forward-only plan (memory "infer"): the class mask uint8
        [B, D, H, W] -- torch.argmax(self(x), 1), first maximum -- then, when ``labels``
        [B, D, H, W] is given, the [K, K + 1] int64 confusion counts of per_class_metrics_3d
        (``ignore_index`` None: no voxel masked), then, when ``return_logits``, the logits
        [B, K, D, H, W].  Where the streaming head covers the plan the logits are never
        written unless asked for."""
        x = _pick_first_if_seq(x)
        E.require_device(x, "UNet3D_SpectralCore.predict")
        plan = self._engine_plan(x, "infer", memory="infer")
        flat = self._ensure_flat(plan, self._engine_params(plan), x.device)
        self._infer_plan = plan
        mask, conf, logits_cl = plan.predict(x.float(), flat, labels, ignore_index,
                                             want_logits=return_logits)
        out = (mask,)
        if labels is not None:
            out += (conf,)
        if return_logits:
            out += (logits_cl.permute(0, 4, 1, 2, 3),)
        return out[0] if len(out) == 1 else out

    @torch.no_grad()
    def predict_tiled(self, x, roi, overlap=0.5, blend="gaussian", sigma_scale=0.125,
                      blend_of="logits", window_batch=1, mirror_axes=(), labels=None,
                      ignore_index=None, return_scores=False):
        """helpers.predict_tiled with the windows on ONE forward-only plan (memory "infer")
        of shape [window_batch, C, roi], its logits written channel-last into one buffer.
        Whatever the forward refuses for the window shape is refused here the same way."""
        x = _pick_first_if_seq(x)
        E.require_device(x, "UNet3D_SpectralCore.predict_tiled")
        held = []

        def forward_cl(stage, out):
            if not held:
                plan = self._engine_plan(stage, "infer", memory="infer")
                held.extend((plan, self._ensure_flat(plan, self._engine_params(plan),
                                                     stage.device)))
                self._infer_plan = plan
            return held[0].forward(stage, held[1], out=out)
        return _predict_tiled(self, x, roi, overlap=overlap, blend=blend, sigma_scale=sigma_scale,
                              blend_of=blend_of, window_batch=window_batch,
                              mirror_axes=mirror_axes, labels=labels, ignore_index=ignore_index,
                              return_scores=return_scores, forward_cl=forward_cl)


def upgrade_spct_with_novel_blocks(m: nn.Module, use_efilm: bool = True, use_fouriergate: bool = True,
                                   use_moe: bool = False, moe_K: int = 3):
    """models.py:1416-1446: replace every _DoubleConvSpectral by the novel block."""
    for name, child in list(m.named_children()):
        if isinstance(child, _DoubleConvSpectral):
            conv1, conv2 = child.b1[0], child.b2[0]
            new_block = _DoubleConvSpectral_Novel(int(conv1.in_channels), int(conv2.out_channels),
                                                  ksd=int(conv1.kernel_size[0]), use_efilm=use_efilm,
                                                  use_fouriergate=use_fouriergate, use_moe=use_moe,
                                                  moe_K=moe_K)
            setattr(m, name, new_block)
        else:
            upgrade_spct_with_novel_blocks(child, use_efilm, use_fouriergate, use_moe, moe_K)
    return m


def build_spct_energyfilm_fourier(num_classes=NUM_CLASSES, base=32, ksd=3, use_se=True, use_specse=True,
                                  use_spatial=False, use_skip_gate=False, in_channels=1, **kw):
    """models.py:1547-1555 (``in_channels`` added for the Cin=5 north-star layout)."""
    core = UNet3D_SpectralCore(in_channels=in_channels, num_classes=num_classes, base=base, ksd=ksd,
                               use_se=use_se, use_specse=use_specse, use_spatial=use_spatial,
                               use_skip_gate=use_skip_gate, **kw)
    return upgrade_spct_with_novel_blocks(core, use_efilm=True, use_fouriergate=True, use_moe=False)


# ----------------------------------------------------------- Lightning layer --
class BaseLitModel(pl.LightningModule):
    """models.py:466-594.  The loss is the fused HIP ce_plus_macro_dice kernel;
    metrics come from its confusion matrix (one host copy instead of ~100
    .item() syncs).  The test-only PR-AUC / ROC-AUC / IoU / precision block
    (models.py:510-584) runs on the device too: helpers.ranking_metrics, the exact
    ranking kernel of csrc/rank.hip in place of scikit-learn, under the reference's key
    names; FAST_SIMPLE_METRICS=1 skips it as in the reference's train.py."""

    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, is_3d=True, **kwargs):
        super().__init__()
        self.is_3d = bool(is_3d)
        self.save_hyperparameters({"num_classes": num_classes, "lr": float(lr), "is_3d": bool(is_3d),
                                   **kwargs})
        self.lambda_esc = float(kwargs.get("lambda_esc", 0.0))
        self.lambda_smooth = float(kwargs.get("lambda_smooth", 0.0))

    def _normalize_input(self, x):
        return _pick_first_if_seq(x)

    def forward(self, x):
        return self.model(self._normalize_input(x))

    def predict(self, x, labels=None, ignore_index=None, return_logits=False):
        """The core's predict (UNet3D_SpectralCore.predict) after forward's input handling"""
        return self.model.predict(self._normalize_input(x), labels=labels,
                                  ignore_index=ignore_index, return_logits=return_logits)

    def predict_tiled(self, x, roi, **kw):
        """The core's predict_tiled (UNet3D_SpectralCore.predict_tiled, same keywords) after
        forward's input handling"""
        return self.model.predict_tiled(self._normalize_input(x), roi, **kw)

    def compute_loss(self, logits, labels):
        return ce_plus_macro_dice_loss(logits, labels, self.hparams.num_classes, ignore_index=IGNORE_INDEX)

    def _shared_step(self, batch, prefix):
        imgs, lbls = _image_label(batch)
        imgs = _pick_first_if_seq(imgs)
        lbls = _pick_first_if_seq(lbls)
        if not self.is_3d:
            lbls = _canonicalize_targets_2d(lbls)
        logits = self(imgs)
        lbls = lbls.to(logits.device).long()
        K = int(self.hparams.num_classes)
        loss, conf = ce_dice_with_confusion(logits, lbls, K, IGNORE_INDEX)
        # per_class_metrics_3d(logits, lbls, K, ignore_index=IGNORE_INDEX) from the same counts
        (dice_list, sens_list, spec_list, macro_dice, macro_sens, macro_spec,
         micro_dice, micro_sens, micro_spec) = metrics_from_confusion(conf.cpu().numpy(), K,
                                                                      int(lbls.numel()))
        self.log(f"{prefix}_loss", loss, on_step=False, on_epoch=True, prog_bar=(prefix == "train"),
                 sync_dist=True)
        self.log(f"{prefix}_macro_dice", macro_dice, on_step=False, on_epoch=True,
                 prog_bar=(prefix != "test"), sync_dist=True)
        for k, v in (("micro_dice", micro_dice), ("macro_sens", macro_sens), ("macro_spec", macro_spec),
                     ("micro_sens", micro_sens), ("micro_spec", micro_spec)):
            self.log(f"{prefix}_{k}", v, on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)
        for i, (d, s, sp) in enumerate(zip(dice_list, sens_list, spec_list)):
            self.log(f"{prefix}_dice_class_{i}", d, on_step=False, on_epoch=True, prog_bar=False, sync_dist=True)
            self.log(f"{prefix}_sens_class_{i}", s, on_step=False, on_epoch=True, prog_bar=False, sync_dist=True)
            self.log(f"{prefix}_spec_class_{i}", sp, on_step=False, on_epoch=True, prog_bar=False, sync_dist=True)
        # the test-only PR / ROC / IoU / precision block (models.py:510-584), 4 K + 8 keys
        if prefix == "test" and not fast_simple_metrics():
            rm = ranking_metrics(logits, lbls, K)
            kw = dict(on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)
            for i in range(K):
                self.log(f"{prefix}_pr_auc_class_{i}", rm["pr_auc"][i], **kw)
                self.log(f"{prefix}_iou_class_{i}", rm["iou"][i], **kw)
                self.log(f"{prefix}_precision_class_{i}", rm["precision"][i], **kw)
                self.log(f"{prefix}_roc_auc_class_{i}", rm["roc_auc"][i], **kw)
            for form in ("macro", "micro"):
                for m in ("pr_auc", "roc_auc", "iou", "precision"):
                    self.log(f"{prefix}_{m}_{form}", rm[f"{m}_{form}"], **kw)
        return loss

    def training_step(self, batch, batch_idx, dataloader_idx=0):
        return self._shared_step(batch, "train")

    def validation_step(self, batch, batch_idx, dataloader_idx=0):
        return {"val_loss": self._shared_step(batch, "val")}

    def test_step(self, batch, batch_idx):
        return self._shared_step(batch, "test")

    def configure_optimizers(self):
        # SPFF_FUSED_ADAM=1: the engine's fused Adam (same arithmetic, one pass)
        if os.environ.get("SPFF_FUSED_ADAM", "0") == "1":
            from .optim import SPFFAdam
            opt = SPFFAdam(self.parameters(), lr=self.hparams.lr)
        else:
            opt = torch.optim.Adam(self.parameters(), lr=self.hparams.lr)
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=5)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sch, "monitor": "val_macro_dice"}}


def supports_predict(model) -> bool:
    """``model.predict`` runs the engine's fused class-mask head: a BaseLitModel with the
    plain forward over a UNet3D_SpectralCore, or that core itself."""
    if isinstance(model, UNet3D_SpectralCore):
        return True
    return (isinstance(model, BaseLitModel) and type(model).forward is BaseLitModel.forward
            and isinstance(getattr(model, "model", None), UNet3D_SpectralCore))


class _LitSPCT_Base(BaseLitModel):
    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, pad_multiple: int = 16):
        super().__init__(num_classes=num_classes, lr=lr, is_3d=True)
        self._pad_multiple = int(pad_multiple)

    def forward(self, x):
        x = _pick_first_if_seq(x)
        if x.ndim == 4:
            x = x.unsqueeze(1)
        x_pad, orig = _pad_to_mult_3d(x, self._pad_multiple)
        return _center_crop_3d(self.model(x_pad), orig)

    def predict(self, x, labels=None, ignore_index=None, return_logits=False):
        raise NotImplementedError("predict: the padded forward of this wrapper crops its logits; "
                                  "the fused head would count the padding's voxels")

    def predict_tiled(self, x, roi, **kw):
        raise NotImplementedError("predict_tiled: the padded forward of this wrapper crops its "
                                  "logits; use helpers.predict_tiled(model, x, roi, ...), which "
                                  "runs the windows through forward")


class LitSPCT_EFiLM_FourierGate(BaseLitModel):
    """The north-star model: registry entry "SPFF-UNet" (config.py:423-428)."""

    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, base=32, ksd=3, use_se=True, use_specse=True,
                 use_spatial=False, use_skip_gate=False, **kw):
        super().__init__(num_classes=num_classes, lr=lr, is_3d=True)
        self.model = build_spct_energyfilm_fourier(num_classes=num_classes, base=base, ksd=ksd,
                                                   use_se=use_se, use_specse=use_specse,
                                                   use_spatial=use_spatial, use_skip_gate=use_skip_gate, **kw)


class LitSPCT_EnergyFiLM(BaseLitModel):
    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, base=32, ksd=3, use_se=True, use_specse=True,
                 use_spatial=False, use_skip_gate=False, in_channels=1, **kw):
        super().__init__(num_classes=num_classes, lr=lr, is_3d=True, **kw)
        core = UNet3D_SpectralCore(in_channels=in_channels, num_classes=num_classes, base=base, ksd=ksd,
                                   use_se=use_se, use_specse=use_specse, use_spatial=use_spatial,
                                   use_skip_gate=use_skip_gate)
        self.model = upgrade_spct_with_novel_blocks(core, use_efilm=True, use_fouriergate=False)


class LitSPCT_FourierGate(BaseLitModel):
    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, base=32, ksd=3, use_se=True, use_specse=True,
                 use_spatial=False, use_skip_gate=False, in_channels=1, **kw):
        super().__init__(num_classes=num_classes, lr=lr, is_3d=True, **kw)
        core = UNet3D_SpectralCore(in_channels=in_channels, num_classes=num_classes, base=base, ksd=ksd,
                                   use_se=use_se, use_specse=use_specse, use_spatial=use_spatial,
                                   use_skip_gate=use_skip_gate)
        self.model = upgrade_spct_with_novel_blocks(core, use_efilm=False, use_fouriergate=True)


class LitSPCT_SEspec(_LitSPCT_Base):
    """Channel-SE + Spectral-SE at all stages (models.py:1585-1592)."""

    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, base=32, pad_multiple=16):
        super().__init__(num_classes=num_classes, lr=lr, pad_multiple=pad_multiple)
        self.model = UNet3D_SpectralCore(in_channels=1, num_classes=num_classes, base=base, ksd=3,
                                         use_se=True, use_specse=True, use_spatial=False,
                                         use_skip_gate=False)


class LitSPCT_ControlUNet(BaseLitModel):
    def __init__(self, num_classes=NUM_CLASSES, lr=BEST_LR, base=32, ksd=3, use_se=False, use_specse=False,
                 use_spatial=False, use_skip_gate=False, in_channels=1, **kw):
        super().__init__(num_classes=num_classes, lr=lr, is_3d=True, **kw)
        self.model = UNet3D_SpectralCore(in_channels=in_channels, num_classes=num_classes, base=base,
                                         ksd=ksd, use_se=use_se, use_specse=use_specse,
                                         use_spatial=use_spatial, use_skip_gate=use_skip_gate)


# ============================================================================
# 3DUNet baseline variant (BASELINE config 3; registry entry "3DUNet",
# config.py:283-311): Cicek3DUNet (models.py:718-753) + the depth-adapter
# Lightning wrapper (models.py:756-853), on the engine's spff_unet3d plan.
# ============================================================================
class Cicek3DUNet(_FlatParamMixin, nn.Module):
    """models.py:718-753.  Same module tree / state-dict keys as the reference
    (enc1.0.weight, enc1.1.running_mean, ..., up4.weight, out.bias); the
    Conv3d / BatchNorm3d children are parameter containers and forward runs on
    the engine (BatchNorm in train mode: batch statistics + running-stat update;
    eval mode: running statistics).  D, H, W must be multiples of 16."""

    def __init__(self, num_classes: int, base: int = 32, use_bn: bool = True, in_channels: int = 1):
        super().__init__()
        if not use_bn:
            raise NotImplementedError("use_bn=False (conv bias + Identity norm) is not on the "
                                      "registry path (config.py:308 sets use_bn=True)")

        def block(ci, co):
            return nn.Sequential(
                nn.Conv3d(ci, co, 3, padding=1, bias=False), nn.BatchNorm3d(co), nn.ReLU(inplace=True),
                nn.Conv3d(co, co, 3, padding=1, bias=False), nn.BatchNorm3d(co), nn.ReLU(inplace=True),
            )
        self.num_classes, self.base, self.in_channels = int(num_classes), int(base), int(in_channels)
        self.enc1 = block(in_channels, base); self.pool1 = nn.MaxPool3d(2)  # noqa: E702
        self.enc2 = block(base, base * 2); self.pool2 = nn.MaxPool3d(2)  # noqa: E702
        self.enc3 = block(base * 2, base * 4); self.pool3 = nn.MaxPool3d(2)  # noqa: E702
        self.enc4 = block(base * 4, base * 8); self.pool4 = nn.MaxPool3d(2)  # noqa: E702
        self.bott = block(base * 8, base * 16)
        self.up4 = nn.ConvTranspose3d(base * 16, base * 8, 2, stride=2)
        self.dec4 = block(base * 8 + base * 8, base * 8)
        self.up3 = nn.ConvTranspose3d(base * 8, base * 4, 2, stride=2)
        self.dec3 = block(base * 4 + base * 4, base * 4)
        self.up2 = nn.ConvTranspose3d(base * 4, base * 2, 2, stride=2)
        self.dec2 = block(base * 2 + base * 2, base * 2)
        self.up1 = nn.ConvTranspose3d(base * 2, base, 2, stride=2)
        self.dec1 = block(base + base, base)
        self.out = nn.Conv3d(base, num_classes, 1)
        self._flat = None
        self._bufs = None

    def _bn_modules(self):
        return [m for m in self.modules() if isinstance(m, nn.BatchNorm3d)]

    def _check_bn(self):
        for m in self._bn_modules():
            if (m.momentum != 0.1 or m.eps != 1e-5 or not m.affine or not m.track_running_stats):
                raise NotImplementedError("engine BatchNorm3d: momentum=0.1, eps=1e-5, affine, "
                                          "track_running_stats (the nn.BatchNorm3d defaults)")

    def _plan(self, x, target_depth: int):
        B, C, D, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"expected {self.in_channels} input channels, got {C}")
        return E.get_unet3d_plan(batch=B, in_ch=C, depth=D, height=H, width=W,
                                 num_classes=self.num_classes, base=self.base,
                                 target_depth=int(target_depth) if target_depth != D else 0,
                                 device=x.device, math=getattr(self, "math", None),
                                 owner=self)

    def _ensure_bufs(self, plan, device):
        named = dict(self.named_buffers())
        bufs = self._bufs
        ok = bufs is not None and bufs.device == device and bufs.numel() == plan.nbuf
        if ok:
            base = bufs.data_ptr()
            ok = all(named[n].data_ptr() == base + 4 * off and named[n].dtype == torch.float32
                     for n, off, _k in plan.buffers)
        if not ok:
            bufs = torch.empty(plan.nbuf, dtype=torch.float32, device=device)
            with torch.no_grad():
                for name, off, n in plan.buffers:
                    b = named[name]
                    bufs[off:off + n].copy_(b.detach().reshape(-1).to(device=device,
                                                                      dtype=torch.float32))
                    b.data = bufs[off:off + n].view(b.shape)
            self._bufs = bufs
            for m in self._bn_modules():  # keep num_batches_tracked next to its stats
                m.num_batches_tracked.data = m.num_batches_tracked.data.to(device)
        return bufs

    def run(self, x, target_depth: int = 0):
        """Forward with the depth adapter fused in (target_depth > 0 resamples D
        there and back, models.py:771-777); returns [B,K,D,H,W] logits."""
        x = _pick_first_if_seq(x)
        E.require_device(x, "Cicek3DUNet.forward")
        self._check_bn()
        plan = self._plan(x, target_depth)
        bufs = self._ensure_bufs(plan, x.device)
        plan.workspace(x.device)
        # data parallelism with synchronised BatchNorm: ``self.sync_bn`` = a collective with
        # allreduce(t) / world over the group (distributed.sync_batchnorm's TorchDepthColl); None:
        # per-replica statistics (DDP without SyncBN, the reference's Lightning default)
        sync = getattr(self, "sync_bn", None)
        if getattr(plan, "_sync_impl", None) is not sync:
            plan.set_sync_bn(sync)
            plan._sync_impl = sync
        training = bool(self.training)
        if training:
            with torch.no_grad():
                for m in self._bn_modules():
                    m.num_batches_tracked.add_(1)
        return self._run_plan(plan, x, (bufs, training))

    def forward(self, x):
        return self.run(x, 0)


class _WeightedCE(_DeviceLoss):
    """(logits, labels, K, ignore_index, class_weights) -> (loss, conf [K, K+1])"""

    WHAT = "weighted softmax CE"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl, conf = E.weighted_ce_forward(lcl, labels, *args)
        return dl, out4[0], conf


class _UNet3DLoss(_DeviceLoss):
    """(logits, labels, K, ignore_index, class_weights, voxel_weights, include_bg, ce_weight,
    dice_weight) -> (loss, out4 = [ce, loss, dice_loss, sum m u]); only the loss carries a
    gradient."""

    WHAT = "3DUNet loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl = E.unet3d_loss_forward(lcl, labels, *args)
        return dl, out4[1].clone(), out4


class LitCicek3DUNet_DepthAdapter_Published(pl.LightningModule):
    """models.py:756-853 (registry "3DUNet", config.py:283-311): depth adapter
    (resample D -> target_depth -> backbone -> back, fused into the engine),
    weighted softmax CE with ignore_index on the fused HIP loss kernel (class
    weights optional; denominator max(N_valid, 1)), macro-Dice logging from its
    confusion counts, SGD(momentum) as configure_optimizers.  Per-voxel CE weights
    (``voxel_weight_key``) and the per-sample soft-Dice term (``dice_weight`` > 0) run as one
    call of the soft-Dice loss driver (_UNet3DLoss)."""

    def __init__(self, num_classes: int, target_depth: int = 16,
                 lr: float = 1e-2, momentum: float = 0.99, nesterov: bool = False,
                 weight_decay: float = 0.0, ignore_index: Optional[int] = 255,
                 class_weights: Optional[List[float]] = None, voxel_weight_key: Optional[str] = None,
                 ce_weight: float = 1.0, dice_weight: float = 0.0, use_bn: bool = True,
                 include_bg_in_dice: bool = False, *args, **kwargs):
        super().__init__()
        self.save_hyperparameters({"num_classes": num_classes, "target_depth": target_depth,
                                   "lr": lr, "momentum": momentum, "nesterov": nesterov,
                                   "weight_decay": weight_decay, "ignore_index": ignore_index,
                                   "class_weights": class_weights,
                                   "voxel_weight_key": voxel_weight_key, "ce_weight": ce_weight,
                                   "dice_weight": dice_weight, "use_bn": use_bn,
                                   "include_bg_in_dice": include_bg_in_dice})
        self.backbone = Cicek3DUNet(num_classes=num_classes, base=32, use_bn=use_bn)
        self.target_depth = int(target_depth)
        if class_weights is not None:
            cw = np.asarray(class_weights, dtype="float32")
            assert cw.shape[0] == int(num_classes)
            self.register_buffer("class_weights", torch.from_numpy(cw), persistent=True)
        else:
            self.class_weights = None
        self.voxel_weight_key = voxel_weight_key
        self.ignore_index = ignore_index
        self.include_bg_in_dice = include_bg_in_dice
        self.ce_weight = float(ce_weight)
        self.dice_weight = float(dice_weight)

    def forward(self, x):
        return self.backbone.run(_pick_first_if_seq(x), self.target_depth)

    def _voxel_weights(self, voxel_weights, target):
        """The weights in the labels' shape (a size-1 channel dimension squeezed), or None.
        The reference would broadcast any other shape silently; here it is an error."""
        if voxel_weights is None:
            return None
        vw = torch.as_tensor(voxel_weights)
        if vw.ndim == target.ndim + 1 and vw.shape[1] == 1:
            vw = vw[:, 0]
        if vw.shape != target.shape:
            raise ValueError(f"voxel weights {tuple(vw.shape)} do not match the labels "
                             f"{tuple(target.shape)}")
        return vw

    def _device_loss(self, logits, target, voxel_weights, ce_weight, dice_weight):
        """One call of the loss driver: (ce_weight ce + dice_weight dice_loss, out4)."""
        if target.ndim == 5 and target.shape[1] == 1:
            target = target[:, 0]
        ign = None if self.ignore_index is None else int(self.ignore_index)
        return _UNet3DLoss.apply(logits, target, int(self.hparams.num_classes), ign,
                                 getattr(self, "class_weights", None),
                                 self._voxel_weights(voxel_weights, target),
                                 bool(self.include_bg_in_dice), float(ce_weight),
                                 float(dice_weight))

    def _weighted_softmax_ce(self, logits, target, voxel_weights: Optional[torch.Tensor]):
        if target.ndim == 5 and target.shape[1] == 1:
            target = target[:, 0]
        if voxel_weights is not None:
            return self._device_loss(logits, target, voxel_weights, 1.0, 0.0)[0]
        ign = self.ignore_index if self.ignore_index is not None else -1000
        loss, conf = _WeightedCE.apply(logits, target, int(self.hparams.num_classes), int(ign),
                                       getattr(self, "class_weights", None))
        self._last_conf = conf
        return loss

    def _dice_loss(self, logits, y, eps=1e-6):
        if eps != 1e-6:
            raise NotImplementedError("the loss kernel's eps is 1e-6")
        return self._device_loss(logits, y, None, 0.0, 1.0)[0]

    def _loss_and_log(self, logits, y, stage: str, voxel_w: Optional[torch.Tensor],
                      log_metrics: bool = True):
        K = int(self.hparams.num_classes)
        if voxel_w is not None or self.dice_weight > 0.0:
            # CE (class and voxel weights) and the soft-Dice term in one pass pair; the
            # argmax counts of the metrics come from their own kernel
            loss, _out4 = self._device_loss(logits, y, voxel_w, self.ce_weight,
                                            max(self.dice_weight, 0.0))
            conf = None
        else:
            loss = self._weighted_softmax_ce(logits, y, None) * self.ce_weight
            conf = self._last_conf
        self.log(f"{stage}_loss", loss, prog_bar=(stage == "train"), on_step=False, on_epoch=True,
                 sync_dist=True)
        if log_metrics:
            # per_class_metrics_3d(logits, tgt, K, ignore_index) from the argmax counts the
            # loss kernel already produced (ignore_index None <-> the loss's -1000: no label
            # equals either, so the counts are the same)
            tgt = _canonicalize_targets_3d(y)
            if conf is None:
                conf = E.confusion(_logits_cl(logits.detach()), tgt.to(logits.device), K,
                                   self.ignore_index)
            met = metrics_from_confusion(conf.cpu().numpy(), K, int(tgt.numel()))
            self.log(f"{stage}_macro_dice", met[3], on_step=False, on_epoch=True, prog_bar=True,
                     sync_dist=True)
        return loss

    def _unpack(self, batch):
        if isinstance(batch, (list, tuple)):
            x, y = batch
            voxel_w = None
        else:
            x, y = batch["image"], batch["label"]
            voxel_w = batch.get(self.voxel_weight_key) if self.voxel_weight_key is not None else None
        return x, y, voxel_w

    def training_step(self, batch, _):
        x, y, vw = self._unpack(batch)
        logits = self(x)
        return self._loss_and_log(logits, y.to(logits.device), "train", voxel_w=vw)

    def validation_step(self, batch, _):
        x, y, vw = self._unpack(batch)
        logits = self(x)
        return self._loss_and_log(logits, y.to(logits.device), "val", voxel_w=vw, log_metrics=True)

    def test_step(self, batch, _):
        x, y, vw = self._unpack(batch)
        logits = self(x)
        return self._loss_and_log(logits, y.to(logits.device), "test", voxel_w=vw)

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=self.hparams.lr,
                               momentum=self.hparams.momentum,
                               nesterov=bool(self.hparams.nesterov),
                               weight_decay=self.hparams.weight_decay)


# ============================================================================
# SwinUNETR variant (BASELINE config 5; registry "SwinUNETR", config.py:366-386):
# LitSwinUNETR_Published (models.py:880-982) around SwinUNETR_Published
# (models.py:858-878), i.e. MONAI 1.5.2 SwinUNETR, on the engine's spff_swin
# plan.  The module tree below only holds parameters under MONAI's state-dict
# names; forward runs on the HIP engine.  Parity unpinned (no MONAI offline):
# semantics in oracle/swin_oracle.py.
# ============================================================================
class _Holder(nn.Module):
    """Parameter container (MONAI module names; no forward)."""


def _conv_holder(conv: nn.Module) -> nn.Module:
    h = _Holder()
    h.conv = conv
    return h


def _res_block(ci: int, co: int) -> nn.Module:
    """MONAI UnetResBlock (conv1.conv, conv2.conv[, conv3.conv]; InstanceNorm3d
    without affine has no parameters)."""
    r = _Holder()
    r.conv1 = _conv_holder(nn.Conv3d(ci, co, 3, padding=1, bias=False))
    r.conv2 = _conv_holder(nn.Conv3d(co, co, 3, padding=1, bias=False))
    if ci != co:
        r.conv3 = _conv_holder(nn.Conv3d(ci, co, 1, bias=False))
    return r


class _WindowAttentionP(nn.Module):
    def __init__(self, dim: int, heads: int, window: int):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * window - 1) ** 3, heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        c = torch.stack(torch.meshgrid(torch.arange(window), torch.arange(window),
                                       torch.arange(window), indexing="ij")).flatten(1)
        r = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (window - 1)
        idx = r[..., 0] * (2 * window - 1) ** 2 + r[..., 1] * (2 * window - 1) + r[..., 2]
        self.register_buffer("relative_position_index", idx)
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)


class _SwinBlockP(nn.Module):
    def __init__(self, dim: int, heads: int, window: int, mlp_ratio: float):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttentionP(dim, heads, window)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Holder()
        self.mlp.linear1 = nn.Linear(dim, int(dim * mlp_ratio))
        self.mlp.linear2 = nn.Linear(int(dim * mlp_ratio), dim)


class _BasicLayerP(nn.Module):
    def __init__(self, dim: int, heads: int, window: int, mlp_ratio: float):
        super().__init__()
        self.blocks = nn.ModuleList([_SwinBlockP(dim, heads, window, mlp_ratio)])
        self.downsample = _Holder()
        self.downsample.reduction = nn.Linear(8 * dim, 2 * dim, bias=False)
        self.downsample.norm = nn.LayerNorm(8 * dim)


class _FlatParamModule(_FlatParamMixin, nn.Module):
    """A MONAI-named parameter tree on one engine plan (SwinUNETR, UNETR)."""


class SwinUNETR(_FlatParamModule):
    """MONAI 1.5.2 SwinUNETR (patch_size 2, depths (1,1,1,1) -- the registry's --,
    normalize=True, res_block, InstanceNorm, downsample "merging", use_v2 False)
    with MONAI's parameter names; forward on the HIP engine (D, H, W multiples
    of 32, as MONAI's _check_input_size requires)."""

    def __init__(self, in_channels: int = 1, out_channels: int = 2, feature_size: int = 24,
                 depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=7,
                 mlp_ratio: float = 4.0, qkv_bias: bool = True, norm_name="instance",
                 drop_rate: float = 0.0, attn_drop_rate: float = 0.0,
                 dropout_path_rate: float = 0.0, normalize: bool = True, use_checkpoint=False,
                 spatial_dims: int = 3, downsample="merging", use_v2: bool = False, **_):
        super().__init__()
        ws = window_size if isinstance(window_size, int) else int(window_size[0])
        if not isinstance(window_size, int) and len(set(window_size)) != 1:
            raise NotImplementedError("cubic windows only")
        if tuple(depths) != (1, 1, 1, 1):
            raise NotImplementedError("depths (1,1,1,1) only (the registry's, config.py:374)")
        if (not qkv_bias or not normalize or use_v2 or downsample != "merging" or spatial_dims != 3
                or str(norm_name).lower() != "instance"):
            raise NotImplementedError("the registry's SwinUNETR settings only (qkv_bias, normalize, "
                                      "merging, instance norm, 3D, use_v2=False)")
        if drop_rate or attn_drop_rate or dropout_path_rate:
            raise NotImplementedError("dropout / drop-path are 0 on the registry path")
        f = int(feature_size)
        self.in_channels, self.num_classes, self.feature_size = int(in_channels), int(out_channels), f
        self.window, self.num_heads, self.mlp_ratio = ws, tuple(int(h) for h in num_heads), float(mlp_ratio)
        self.swinViT = _Holder()
        self.swinViT.patch_embed = _Holder()
        self.swinViT.patch_embed.proj = nn.Conv3d(in_channels, f, 2, stride=2)
        for s in range(4):
            setattr(self.swinViT, f"layers{s + 1}",
                    nn.ModuleList([_BasicLayerP(f << s, self.num_heads[s], ws, mlp_ratio)]))
        self.encoder1 = _Holder(); self.encoder1.layer = _res_block(in_channels, f)  # noqa: E702
        self.encoder2 = _Holder(); self.encoder2.layer = _res_block(f, f)  # noqa: E702
        self.encoder3 = _Holder(); self.encoder3.layer = _res_block(2 * f, 2 * f)  # noqa: E702
        self.encoder4 = _Holder(); self.encoder4.layer = _res_block(4 * f, 4 * f)  # noqa: E702
        self.encoder10 = _Holder(); self.encoder10.layer = _res_block(16 * f, 16 * f)  # noqa: E702
        for name, ci, co in (("decoder5", 16 * f, 8 * f), ("decoder4", 8 * f, 4 * f),
                             ("decoder3", 4 * f, 2 * f), ("decoder2", 2 * f, f), ("decoder1", f, f)):
            d = _Holder()
            d.transp_conv = _conv_holder(nn.ConvTranspose3d(ci, co, 2, stride=2, bias=False))
            d.conv_block = _res_block(2 * co, co)
            setattr(self, name, d)
        self.out = _Holder()
        self.out.conv = _conv_holder(nn.Conv3d(f, out_channels, 1, bias=True))
        self._flat = None

    def _plan(self, x):
        B, C, D, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"expected {self.in_channels} input channels, got {C}")
        if D % 32 or H % 32 or W % 32:
            raise ValueError(f"spatial dims {(D, H, W)} must be divisible by 2**5 = 32")
        return E.get_swin_plan(batch=B, in_ch=C, depth=D, height=H, width=W,
                               num_classes=self.num_classes, feature_size=self.feature_size,
                               window=self.window, heads=self.num_heads, mlp_ratio=self.mlp_ratio,
                               device=x.device, math=getattr(self, "math", None),
                               owner=self)

    def forward(self, x_in):
        E.require_device(x_in, "SwinUNETR.forward")
        return self._run_plan(self._plan(x_in), x_in)


class SwinUNETR_Published(nn.Module):
    """models.py:858-878: builds SwinUNETR with the kwargs MONAI 1.5.2 accepts
    (img_size dropped, drop_path_rate -> dropout_path_rate, spatial_dims=3)."""

    def __init__(self, num_classes, img_size=(96, 96, 96), in_channels=1, feature_size=48,
                 depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), mlp_ratio=4.0, drop_rate=0.0,
                 attn_drop_rate=0.0, dropout_path_rate=0.0, use_checkpoint=False,
                 norm_name="instance", **kwargs):
        super().__init__()
        self.model = SwinUNETR(in_channels=in_channels, out_channels=num_classes,
                               feature_size=feature_size, depths=depths, num_heads=num_heads,
                               mlp_ratio=mlp_ratio, drop_rate=drop_rate,
                               attn_drop_rate=attn_drop_rate, dropout_path_rate=dropout_path_rate,
                               use_checkpoint=use_checkpoint, norm_name=norm_name, spatial_dims=3)

    def forward(self, x):
        return self.model(x)


class _SwinLoss(_DeviceLoss):
    """(logits, labels, K, ignore_index, include_bg, ce_weight) -> loss"""

    WHAT = "SwinUNETR loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl = E.swin_loss_forward(lcl, labels, *args)
        return dl, out4[1]


class _DiceCEWarmupLit(pl.LightningModule):
    """What LitSwinUNETR_Published and LitUNETR_Published share in the reference
    (models.py:906-982 and 1038-1115 are the same code): the (1 - w) soft-Dice + w CE
    loss on the fused HIP loss kernels, the linear warm-up + cosine learning rate, the
    step methods and AdamW.  Subclasses set hparams, _total_train_iters / _iters_done
    and forward."""

    def _loss(self, logits, labels):
        if labels.ndim == 5 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if not self.hparams.use_ce_alongside_dice:
            raise NotImplementedError("dice-only loss is off on the registry path (config.py:383)")
        ign = self.hparams.ignore_index
        return _SwinLoss.apply(logits, labels, int(logits.shape[1]),
                               int(ign) if ign is not None else -1000,
                               bool(self.hparams.include_bg_in_dice), float(self.hparams.ce_weight))

    def on_train_batch_start(self, batch, batch_idx):
        """linear warm-up then cosine decay of the learning rate (models.py:941-951)."""
        tr = getattr(self, "trainer", None)
        nb = int(getattr(tr, "num_training_batches", 0) or 1) if tr is not None else 1
        warmup_iters = int(self.hparams.warmup_epochs * nb)
        t, T = self._iters_done, max(1, self._total_train_iters or 1)
        if t < warmup_iters:
            lr = self.hparams.lr * float(t + 1) / max(1, warmup_iters)
        else:
            prog = (t - warmup_iters) / max(1, T - warmup_iters)
            lr = 0.5 * self.hparams.lr * (1.0 + math.cos(math.pi * prog))
        opt = self.optimizers() if hasattr(self, "optimizers") and tr is not None else None
        if opt:
            for pg in opt.param_groups:
                pg["lr"] = lr
        return lr

    def on_train_batch_end(self, outputs, batch, batch_idx):
        self._iters_done += 1

    def _step(self, batch, stage):
        imgs, lbls = _image_label(batch)
        logits = self(imgs)
        tgt = _canonicalize_targets_3d(lbls).to(logits.device)
        loss = self._loss(logits, tgt)
        met = per_class_metrics_3d(logits, tgt, self.hparams.num_classes,
                                   ignore_index=self.hparams.ignore_index)
        self.log(f"{stage}_loss", loss, on_epoch=True, prog_bar=True, sync_dist=True)
        self.log(f"{stage}_macro_dice", met[3], on_epoch=True, prog_bar=True, sync_dist=True)
        self.log(f"{stage}_micro_dice", met[6], on_epoch=True, prog_bar=False, sync_dist=True)
        return loss

    def training_step(self, batch, _):
        return self._step(batch, "train")

    def validation_step(self, batch, _):
        return self._step(batch, "val")

    def test_step(self, batch, _):
        return self._step(batch, "test")

    def configure_optimizers(self):
        return torch.optim.AdamW(self.parameters(), lr=self.hparams.lr,
                                 weight_decay=self.hparams.weight_decay, betas=(0.9, 0.999))


class LitSwinUNETR_Published(_DiceCEWarmupLit):
    """models.py:880-982 (registry "SwinUNETR"): pad to a multiple of 32 (replicate,
    centred) -> SwinUNETR -> crop; loss (1 - w) soft-Dice + w CE(ignore) on the
    fused HIP loss kernels; AdamW with linear warm-up + cosine decay."""

    def __init__(self, num_classes: int, img_size=(96, 96, 96), in_channels: int = 1,
                 feature_size: int = 48, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24),
                 mlp_ratio: float = 4.0, drop_rate: float = 0.0, attn_drop_rate: float = 0.0,
                 dropout_path_rate: float = 0.0, use_checkpoint: bool = False,
                 norm_name: str = "instance", lr: float = 1e-4, weight_decay: float = 1e-2,
                 warmup_epochs: int = 5, use_ce_alongside_dice: bool = True,
                 ce_weight: float = 0.5, ignore_index: Optional[int] = IGNORE_INDEX,
                 include_bg_in_dice: bool = True):
        super().__init__()
        self.save_hyperparameters({
            "num_classes": num_classes, "img_size": img_size, "in_channels": in_channels,
            "feature_size": feature_size, "depths": depths, "num_heads": num_heads,
            "mlp_ratio": mlp_ratio, "drop_rate": drop_rate, "attn_drop_rate": attn_drop_rate,
            "dropout_path_rate": dropout_path_rate, "use_checkpoint": use_checkpoint,
            "norm_name": norm_name, "lr": lr, "weight_decay": weight_decay,
            "warmup_epochs": warmup_epochs, "use_ce_alongside_dice": use_ce_alongside_dice,
            "ce_weight": ce_weight, "ignore_index": ignore_index,
            "include_bg_in_dice": include_bg_in_dice})
        self.model = SwinUNETR_Published(
            num_classes, img_size=img_size, in_channels=in_channels, feature_size=feature_size,
            depths=depths, num_heads=num_heads, mlp_ratio=mlp_ratio, drop_rate=drop_rate,
            attn_drop_rate=attn_drop_rate, dropout_path_rate=dropout_path_rate,
            use_checkpoint=use_checkpoint, norm_name=norm_name)
        self._total_train_iters = None
        self._iters_done = 0

    def forward(self, x):
        x = _pick_first_if_seq(x)
        if x.ndim == 4:
            x = x.unsqueeze(1)
        x_pad, orig = _pad_to_mult_3d(x, 32)
        y_pad = self.model(x_pad)
        return _center_crop_3d(y_pad, orig)


# ============================================================================
# UNETR (registry "UNETR", config.py:316-339): LitUNETR_Published (models.py:
# 1006-1115) around UNETR_Published (987-1004), i.e. MONAI 1.5.2's UNETR, on the
# engine's spff_unetr plan (csrc/unetr.hip).  PARITY UNPINNED: MONAI is not
# available offline; its semantics are restated in tests/_unetr_oracle.py.
# ============================================================================
class _ViTBlockP(nn.Module):
    """MONAI TransformerBlock's parameters in its registration order.  norm_cross_attn and
    cross_attn are registered by MONAI >= 1.4 in every block and never used without
    with_cross_attention: held here so that a MONAI checkpoint loads strictly, outside the
    engine's flat buffer, their gradients stay None."""

    def __init__(self, hidden: int, mlp_dim: int):
        super().__init__()
        self.mlp = _Holder()
        self.mlp.linear1 = nn.Linear(hidden, mlp_dim)
        self.mlp.linear2 = nn.Linear(mlp_dim, hidden)
        self.norm1 = nn.LayerNorm(hidden)
        self.attn = _Holder()
        self.attn.out_proj = nn.Linear(hidden, hidden)
        self.attn.qkv = nn.Linear(hidden, 3 * hidden, bias=False)
        self.norm2 = nn.LayerNorm(hidden)
        self.norm_cross_attn = nn.LayerNorm(hidden)
        self.cross_attn = _Holder()
        self.cross_attn.out_proj = nn.Linear(hidden, hidden)
        self.cross_attn.to_q = nn.Linear(hidden, hidden, bias=False)
        self.cross_attn.to_k = nn.Linear(hidden, hidden, bias=False)
        self.cross_attn.to_v = nn.Linear(hidden, hidden, bias=False)


def _transp_holder(ci: int, co: int) -> nn.Module:
    return _conv_holder(nn.ConvTranspose3d(ci, co, 2, stride=2, bias=False))


def _prup_block(hidden: int, co: int, num_layer: int) -> nn.Module:
    """MONAI UnetrPrUpBlock (conv_block and res_block on)."""
    b = _Holder()
    b.transp_conv_init = _transp_holder(hidden, co)
    b.blocks = nn.ModuleList([nn.ModuleList([_transp_holder(co, co), _res_block(co, co)])
                              for _ in range(num_layer)])
    return b


class UNETR(_FlatParamModule):
    """MONAI 1.5.2 UNETR (conv patch embedding of 16^3, learnable position embedding, twelve
    ViT blocks, InstanceNorm, conv_block and res_block, no dropout, no qkv bias) with MONAI's
    parameter names and constructor signature; forward on the HIP engine."""

    def __init__(self, in_channels: int, out_channels: int, img_size=(96, 96, 96),
                 feature_size: int = 16, hidden_size: int = 768, mlp_dim: int = 3072,
                 num_heads: int = 12, proj_type: str = "conv", norm_name="instance",
                 conv_block: bool = True, res_block: bool = True, dropout_rate: float = 0.0,
                 spatial_dims: int = 3, qkv_bias: bool = False, save_attn: bool = False):
        super().__init__()
        if isinstance(img_size, int):
            img_size = (img_size,) * 3
        if (proj_type != "conv" or not conv_block or not res_block or qkv_bias or spatial_dims != 3
                or str(norm_name).lower() != "instance"):
            raise NotImplementedError("the registry's UNETR settings only (conv patch projection, "
                                      "conv_block, res_block, instance norm, 3D, no qkv bias)")
        if dropout_rate:
            raise NotImplementedError("dropout is 0 on the registry path")
        if hidden_size % num_heads:
            raise ValueError("hidden_size should be divisible by num_heads.")
        if any(int(v) % 16 for v in img_size):
            raise ValueError("img_size should be divisible by the 16^3 patch")
        f, hid = int(feature_size), int(hidden_size)
        self.in_channels, self.num_classes, self.feature_size = int(in_channels), int(out_channels), f
        self.img_size = tuple(int(v) for v in img_size)
        self.hidden_size, self.mlp_dim, self.num_heads = hid, int(mlp_dim), int(num_heads)
        n = (self.img_size[0] // 16) * (self.img_size[1] // 16) * (self.img_size[2] // 16)
        self.vit = _Holder()
        self.vit.patch_embedding = _Holder()
        self.vit.patch_embedding.position_embeddings = nn.Parameter(torch.zeros(1, n, hid))
        nn.init.trunc_normal_(self.vit.patch_embedding.position_embeddings, std=0.02)
        self.vit.patch_embedding.patch_embeddings = nn.Conv3d(in_channels, hid, 16, stride=16)
        self.vit.blocks = nn.ModuleList([_ViTBlockP(hid, self.mlp_dim) for _ in range(12)])
        self.vit.norm = nn.LayerNorm(hid)
        self.encoder1 = _Holder(); self.encoder1.layer = _res_block(in_channels, f)  # noqa: E702
        self.encoder2 = _prup_block(hid, 2 * f, 2)
        self.encoder3 = _prup_block(hid, 4 * f, 1)
        self.encoder4 = _prup_block(hid, 8 * f, 0)
        for name, ci, co in (("decoder5", hid, 8 * f), ("decoder4", 8 * f, 4 * f),
                             ("decoder3", 4 * f, 2 * f), ("decoder2", 2 * f, f)):
            d = _Holder()
            d.transp_conv = _transp_holder(ci, co)
            d.conv_block = _res_block(2 * co, co)
            setattr(self, name, d)
        self.out = _Holder()
        self.out.conv = _conv_holder(nn.Conv3d(f, out_channels, 1, bias=True))
        self._flat = None

    def _plan(self, x):
        B, C, D, H, W = x.shape
        if C != self.in_channels:
            raise ValueError(f"expected {self.in_channels} input channels, got {C}")
        if D % 16 or H % 16 or W % 16:
            raise ValueError(f"spatial dims {(D, H, W)} must be divisible by 16")
        return E.get_unetr_plan(batch=B, in_ch=C, depth=D, height=H, width=W,
                                num_classes=self.num_classes, img=self.img_size,
                                feature_size=self.feature_size, hidden=self.hidden_size,
                                mlp_dim=self.mlp_dim, heads=self.num_heads, device=x.device,
                                math=getattr(self, "math", None), owner=self)

    def run(self, x_in):
        """x_in [B, Cin, D, H, W], multiples of 16.  Another size than img_size is resampled
        to img_size and the logits back (trilinear, align_corners=False) inside the engine:
        steps 3-5 of LitUNETR_Published.forward."""
        E.require_device(x_in, "UNETR.forward")
        return self._run_plan(self._plan(x_in), x_in)

    def forward(self, x_in):
        if tuple(x_in.shape[2:]) != self.img_size:
            raise ValueError(f"UNETR takes inputs of img_size {self.img_size} (the position "
                             f"embedding is tied to it); got {tuple(x_in.shape[2:])}")
        return self.run(x_in)


class UNETR_Published(nn.Module):
    """models.py:987-1004: builds UNETR with the kwargs MONAI 1.5.2 accepts (pos_embed is
    not one of them, so the patch projection is MONAI's default "conv")."""

    def __init__(self, num_classes, img_size=(96, 96, 96), in_channels=1, feature_size=16,
                 hidden_size=768, mlp_dim=3072, num_heads=12, pos_embed="perceptron",
                 norm_name="instance", res_block=True, dropout_rate=0.0):
        super().__init__()
        self.net = UNETR(img_size=img_size, in_channels=in_channels, out_channels=num_classes,
                         feature_size=feature_size, hidden_size=hidden_size, mlp_dim=mlp_dim,
                         num_heads=num_heads, norm_name=norm_name, res_block=res_block,
                         dropout_rate=dropout_rate, spatial_dims=3)

    def forward(self, x):
        return self.net(x)


class LitUNETR_Published(_DiceCEWarmupLit):
    """models.py:1006-1115 (registry "UNETR"): pad to a multiple of 16 (replicate, centred)
    -> resample to img_size when the padded size differs -> UNETR -> resample the logits
    back -> crop; the loss, learning-rate schedule and AdamW of LitSwinUNETR_Published."""

    def __init__(self, num_classes: int, img_size=(96, 96, 96), in_channels: int = 1,
                 feature_size: int = 16, hidden_size: int = 768, mlp_dim: int = 3072,
                 num_heads: int = 12, pos_embed: str = "perceptron", norm_name: str = "instance",
                 res_block: bool = True, dropout_rate: float = 0.0, lr: float = 1e-4,
                 weight_decay: float = 1e-2, warmup_epochs: int = 5,
                 use_ce_alongside_dice: bool = True, ce_weight: float = 0.5,
                 ignore_index: Optional[int] = None, include_bg_in_dice: bool = True):
        super().__init__()
        self.save_hyperparameters({
            "num_classes": num_classes, "img_size": img_size, "in_channels": in_channels,
            "feature_size": feature_size, "hidden_size": hidden_size, "mlp_dim": mlp_dim,
            "num_heads": num_heads, "pos_embed": pos_embed, "norm_name": norm_name,
            "res_block": res_block, "dropout_rate": dropout_rate, "lr": lr,
            "weight_decay": weight_decay, "warmup_epochs": warmup_epochs,
            "use_ce_alongside_dice": use_ce_alongside_dice, "ce_weight": ce_weight,
            "ignore_index": ignore_index, "include_bg_in_dice": include_bg_in_dice})
        self.net = UNETR_Published(num_classes=num_classes, img_size=img_size,
                                   in_channels=in_channels, feature_size=feature_size,
                                   hidden_size=hidden_size, mlp_dim=mlp_dim, num_heads=num_heads,
                                   pos_embed=pos_embed, norm_name=norm_name, res_block=res_block,
                                   dropout_rate=dropout_rate)
        self._total_train_iters = None
        self._iters_done = 0

    def forward(self, x):
        x = _pick_first_if_seq(x)
        if x.ndim == 4:
            x = x.unsqueeze(1)
        x_pad, orig = _pad_to_mult_3d(x)
        y_pad = self.net.net.run(x_pad)
        return _center_crop_3d(y_pad, orig)


# ============================================================================
# R2UNet3D (registry "R2UNet3D"): LitR2UNet3D_Published around
# R2UNet3D_backbone, the recurrent residual 3D U-Net, on the engine's spff_r2u
# plan (csrc/r2unet.hip).  The module tree below only holds parameters under the
# reference's state-dict names; backbone and head run as one plan from the Lit
# module's forward.  Parity: tests/golden/r2u_*.npz.
# ============================================================================
class _RecurrentUnit3D(nn.Module):
    """t steps of relu(InstanceNorm(conv3x3x3(out + h))) with one shared conv and norm."""

    def __init__(self, channels: int, t: int = 2):
        super().__init__()
        self.t = int(t)
        self.conv = nn.Conv3d(channels, channels, 3, padding=1, bias=False)
        self.inn = nn.InstanceNorm3d(channels, affine=True)
        self.act = nn.ReLU(inplace=True)


class _RRCNNBlock3D(nn.Module):
    """x1 = inp(x); o = relu(InstanceNorm(x1 + out(ru(x1)))), inp / out 1x1x1 without bias."""

    def __init__(self, cin: int, cout: int, t: int = 2):
        super().__init__()
        self.inp = nn.Conv3d(cin, cout, 1, bias=False)
        self.ru = _RecurrentUnit3D(cout, t=t)
        self.out = nn.Conv3d(cout, cout, 1, bias=False)
        self.bn = nn.InstanceNorm3d(cout, affine=True)
        self.act = nn.ReLU(inplace=True)


class R2UNet3D_backbone(nn.Module):
    """Five levels of recurrent residual blocks (channels base * {1, 2, 4, 8, 16}),
    MaxPool3d(2) down, ConvTranspose3d(2, stride 2) + cat([up, skip]) up.  A parameter
    container: the engine plan covers backbone and head together, so it runs from
    LitR2UNet3D_Published.forward."""

    def __init__(self, in_channels: int = 1, base: int = 16, t: int = 2):
        super().__init__()
        c = [base, base * 2, base * 4, base * 8, base * 16]
        self.in_channels, self.base, self.t = int(in_channels), int(base), int(t)
        self.e1 = _RRCNNBlock3D(in_channels, c[0], t=t); self.p1 = nn.MaxPool3d(2)  # noqa: E702
        self.e2 = _RRCNNBlock3D(c[0], c[1], t=t); self.p2 = nn.MaxPool3d(2)  # noqa: E702
        self.e3 = _RRCNNBlock3D(c[1], c[2], t=t); self.p3 = nn.MaxPool3d(2)  # noqa: E702
        self.e4 = _RRCNNBlock3D(c[2], c[3], t=t); self.p4 = nn.MaxPool3d(2)  # noqa: E702
        self.b = _RRCNNBlock3D(c[3], c[4], t=t)
        for i, n in ((3, "4"), (2, "3"), (1, "2"), (0, "1")):
            setattr(self, "up" + n, nn.ConvTranspose3d(c[i + 1], c[i], 2, 2))
            setattr(self, "d" + n, _RRCNNBlock3D(c[i] + c[i], c[i], t=t))
        self.out_ch = c[0]

    def forward(self, x):
        raise NotImplementedError("R2UNet3D_backbone holds parameters only: the engine plan runs "
                                  "backbone and head together (LitR2UNet3D_Published.forward)")


class _R2UDiceLoss(_DeviceLoss):
    """(logits, labels, K, ignore_index) -> (loss, out4 = [dice, loss, kept, N_valid]) of the
    foreground-only soft Dice; only the loss carries a gradient."""

    WHAT = "R2UNet3D loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl = E.r2u_dice_loss_forward(lcl, labels, *args)
        return dl, out4[1].clone(), out4


class _PadCropPlanLit(_FlatParamMixin, pl.LightningModule):
    """What LitR2UNet3D_Published and LitResUNetPP3D_Published share: replicate-pad D, H, W
    to multiples of ``hparams.pad_multiple`` -> ``backbone`` and ``head`` as one engine plan
    -> centre crop; the step methods and Adam.  Subclasses build backbone and head and give
    ``_get_plan(**kw)`` (their E.get_*_plan with their own keywords added) and ``_step``."""

    def _plan(self, x):
        B, C, D, H, W = x.shape
        if C != self.backbone.in_channels:
            raise ValueError(f"expected {self.backbone.in_channels} input channels, got {C}")
        return self._get_plan(batch=B, in_ch=C, depth=D, height=H, width=W,
                              num_classes=int(self.hparams.num_classes), device=x.device,
                              math=getattr(self, "math", None), owner=self)

    def forward(self, x):
        x = _pick_first_if_seq(x)
        E.require_device(x, f"{type(self).__name__}.forward")
        if x.ndim == 4:
            x = x.unsqueeze(1)
        m = int(self.hparams.pad_multiple)
        if m % 16:
            raise NotImplementedError("pad_multiple must be a multiple of 16 (four poolings)")
        x_pad, orig = _pad_to_mult_3d(x.float(), m)
        return _center_crop_3d(self._run_plan(self._plan(x_pad), x_pad), orig)

    def training_step(self, batch, _):
        return self._step(batch, "train")

    def validation_step(self, batch, _):
        return self._step(batch, "val")

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=self.hparams.lr,
                                weight_decay=self.hparams.weight_decay)


class LitR2UNet3D_Published(_PadCropPlanLit):
    """Registry "R2UNet3D": replicate-pad D, H, W to multiples of ``pad_multiple`` ->
    R2UNet3D_backbone -> 1x1x1 head -> centre crop (padding and cropping are torch
    plumbing, backbone and head one engine plan); foreground-only soft-Dice loss over the
    samples that have foreground, on the HIP loss kernels; Adam.  ``math`` (attribute)
    selects the conv arithmetic of new plans.  ``num_classes == 1`` (the reference's sigmoid
    branch) is not built."""

    def __init__(self, num_classes: int, in_channels: int = 1, base_features: int = 16, t: int = 2,
                 lr: float = 1e-3, weight_decay: float = 0.0, pad_multiple: int = 16,
                 ignore_index: Optional[int] = None):
        super().__init__()
        if int(num_classes) == 1:
            raise NotImplementedError("LitR2UNet3D_Published: num_classes == 1 (single-channel "
                                      "sigmoid Dice) is not built on the engine; use >= 2 classes")
        self.save_hyperparameters({
            "num_classes": num_classes, "in_channels": in_channels,
            "base_features": base_features, "t": t, "lr": lr, "weight_decay": weight_decay,
            "pad_multiple": pad_multiple, "ignore_index": ignore_index})
        self.backbone = R2UNet3D_backbone(in_channels=in_channels, base=base_features, t=t)
        self.binary = False
        self.head = nn.Conv3d(self.backbone.out_ch, num_classes, 1)
        self._flat = None

    def _get_plan(self, **kw):
        return E.get_r2u_plan(base=self.backbone.base, t=self.backbone.t, **kw)

    @staticmethod
    def _dice_only_loss_with_logits(logits, y, ignore_index=None, eps=1e-6):
        """Foreground-only soft Dice over the samples with foreground: (loss, dice_mean);
        both 0 (and no gradient) when no sample has foreground."""
        if eps != 1e-6:
            raise NotImplementedError("the loss kernel's eps is 1e-6")
        if logits.shape[1] == 1:
            raise NotImplementedError("the single-channel sigmoid Dice branch is not built")
        if y.ndim == 5 and y.size(1) == 1:
            y = y[:, 0]
        loss, out4 = _R2UDiceLoss.apply(logits, y, int(logits.shape[1]),
                                        None if ignore_index is None else int(ignore_index))
        return loss, out4[0]

    def _step(self, batch, stage):
        x, y = _image_label(batch)
        logits = self(x)
        y = torch.as_tensor(y).to(logits.device)
        loss, dice = self._dice_only_loss_with_logits(logits, y,
                                                      ignore_index=self.hparams.ignore_index)
        self.log(f"{stage}_loss", loss, on_epoch=True, prog_bar=True, sync_dist=True)
        self.log(f"{stage}_macro_dice", dice, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss


# ============================================================================
# ResUNet++ (registry "ResUNet++"): LitResUNetPP3D_Published around
# ResUNetPP3D_backbone -- residual units, an ASPP bottleneck, SE on the skips and
# attention gates at the concats -- on the engine's spff_rupp plan
# (csrc/resunetpp.hip).  The module tree below only holds parameters under the
# reference's state-dict names; backbone and head run as one plan from the Lit
# module's forward.  Parity: tests/golden/rupp_*.npz.
# ============================================================================
class ResidualUnit3D(nn.Module):
    """out = relu(IN2(c2(relu(IN1(c1(x))))) + skip(x)); skip is a bias-free 1x1x1 conv, or
    the identity when cin == cout."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.c1 = nn.Conv3d(cin, cout, 3, padding=1, bias=False)
        self.n1 = nn.InstanceNorm3d(cout, affine=True)
        self.c2 = nn.Conv3d(cout, cout, 3, padding=1, bias=False)
        self.n2 = nn.InstanceNorm3d(cout, affine=True)
        self.act = nn.ReLU(inplace=True)
        self.skip = nn.Conv3d(cin, cout, 1, bias=False) if cin != cout else nn.Identity()


class ASPP3D(nn.Module):
    """Four bias-free 3x3x3 convs of one input (dilation = padding = d), concatenated in
    branch order, then a bias-free 1x1x1 conv and a ReLU."""

    def __init__(self, in_channels: int, out_channels: int, dilations=(1, 2, 4, 8)):
        super().__init__()
        self.branches = nn.ModuleList([
            nn.Conv3d(in_channels, out_channels, 3, padding=d, dilation=d, bias=False)
            for d in dilations])
        self.proj = nn.Sequential(
            nn.Conv3d(len(dilations) * out_channels, out_channels, 1, bias=False),
            nn.ReLU(inplace=True))


class SE3D(nn.Module):
    """x * sigmoid(W2 relu(W1 mean(x) + b1) + b2), hidden = max(1, channels // reduction)."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        hidden = max(1, channels // reduction)
        self.pool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Sequential(nn.Conv3d(channels, hidden, 1, bias=True), nn.ReLU(inplace=True),
                                nn.Conv3d(hidden, channels, 1, bias=True), nn.Sigmoid())


class AttentionGate3d(nn.Module):
    """forward(x_skip, g) = x_skip * sigmoid(psi(relu(W_x x_skip + W_g g))): the gate
    multiplies its first argument."""

    def __init__(self, g_c: int, x_c: int, inter_c: Optional[int] = None):
        super().__init__()
        if inter_c is None:
            inter_c = min(x_c, g_c)
        self.W_x = nn.Conv3d(x_c, inter_c, 1, 1, 0, bias=True)
        self.W_g = nn.Conv3d(g_c, inter_c, 1, 1, 0, bias=True)
        self.psi = nn.Conv3d(inter_c, 1, 1, 1, 0, bias=True)
        nn.init.constant_(self.psi.bias, 0.0)
        self.relu = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()


class ResUNetPP3D_backbone(nn.Module):
    """Residual-unit encoder (channels base * {1, 2, 4, 8, 16}, MaxPool3d(2)), ASPP
    bottleneck, SE on the encoder outputs and an attention gate at each concat but the
    last.  The backbone calls ``ag(u, se(e))``, so the gate scales the up-sampled tensor and
    the decoder reads cat([u, u * att]).  A parameter container: the engine plan covers
    backbone and head together, so it runs from LitResUNetPP3D_Published.forward."""

    def __init__(self, in_channels: int = 1, base: int = 16):
        super().__init__()
        c = [base, base * 2, base * 4, base * 8, base * 16]
        self.in_channels, self.base = int(in_channels), int(base)
        self.e1 = ResidualUnit3D(in_channels, c[0]); self.p1 = nn.MaxPool3d(2)  # noqa: E702
        self.e2 = ResidualUnit3D(c[0], c[1]); self.p2 = nn.MaxPool3d(2)  # noqa: E702
        self.e3 = ResidualUnit3D(c[1], c[2]); self.p3 = nn.MaxPool3d(2)  # noqa: E702
        self.e4 = ResidualUnit3D(c[2], c[3]); self.p4 = nn.MaxPool3d(2)  # noqa: E702
        self.b_aspp_in = ResidualUnit3D(c[3], c[4])
        self.b_aspp = ASPP3D(c[4], c[4])
        self.b_aspp_out = ResidualUnit3D(c[4], c[4])
        for i in range(4):
            setattr(self, f"se{i + 1}", SE3D(c[i]))
        for i, n in ((3, "4"), (2, "3"), (1, "2"), (0, "1")):
            setattr(self, "up" + n, nn.ConvTranspose3d(c[i + 1], c[i], 2, 2))
            if i > 0:
                setattr(self, "ag" + n, AttentionGate3d(g_c=c[i], x_c=c[i], inter_c=c[i] // 2))
            setattr(self, "d" + n, ResidualUnit3D(c[i] + c[i], c[i]))
        self.out_ch = c[0]

    def forward(self, x):
        raise NotImplementedError("ResUNetPP3D_backbone holds parameters only: the engine plan "
                                  "runs backbone and head together "
                                  "(LitResUNetPP3D_Published.forward)")


class _RUPPLoss(_DeviceLoss):
    """(logits, labels, K, ignore_index, include_bg, ce_weight, dice_weight) ->
    (loss, out4 = [ce, loss, dice_mean, N_valid]); only the loss carries a gradient."""

    WHAT = "ResUNet++ loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl = E.rupp_loss_forward(lcl, labels, *args)
        return dl, out4[1].clone(), out4


class LitResUNetPP3D_Published(_PadCropPlanLit):
    """Registry "ResUNet++": replicate-pad D, H, W to multiples of ``pad_multiple`` ->
    ResUNetPP3D_backbone -> 1x1x1 head -> centre crop (padding and cropping are torch
    plumbing, backbone and head one engine plan); batch-pooled soft Dice + CE on the HIP loss
    kernels; Adam.  ``math`` (attribute) selects the conv arithmetic of new plans."""

    def __init__(self, num_classes: int, in_channels: int = 1, base_features: int = 16,
                 include_bg_in_dice: bool = False, ignore_index: Optional[int] = None,
                 ce_weight: float = 0.5, dice_weight: float = 0.5, lr: float = 1e-3,
                 weight_decay: float = 1e-5, pad_multiple: int = 16):
        super().__init__()
        if int(num_classes) == 1:
            raise NotImplementedError("LitResUNetPP3D_Published: num_classes == 1 is not built "
                                      "on the engine (the loss kernels take 2..32 classes)")
        if int(pad_multiple) < 16 or int(pad_multiple) % 16:
            raise NotImplementedError("LitResUNetPP3D_Published: pad_multiple must be a multiple "
                                      "of 16 (four poolings whose outputs are concatenated with "
                                      "the up-convolutions)")
        self.save_hyperparameters({
            "num_classes": num_classes, "in_channels": in_channels,
            "base_features": base_features, "include_bg_in_dice": include_bg_in_dice,
            "ignore_index": ignore_index, "ce_weight": ce_weight, "dice_weight": dice_weight,
            "lr": lr, "weight_decay": weight_decay, "pad_multiple": pad_multiple})
        self.backbone = ResUNetPP3D_backbone(in_channels=in_channels, base=base_features)
        self.head = nn.Conv3d(self.backbone.out_ch, num_classes, 1)
        self._flat = None

    def _get_plan(self, **kw):
        return E.get_rupp_plan(base=self.backbone.base, **kw)

    def _loss(self, logits, y):
        """dice_ce_loss_with_metrics: (loss, macro_dice, ce); Dice sums pooled over the batch."""
        hp = self.hparams
        if y.ndim == 5 and y.size(1) == 1:
            y = y[:, 0]
        loss, out4 = _RUPPLoss.apply(
            logits, y, int(logits.shape[1]),
            None if hp.ignore_index is None else int(hp.ignore_index),
            bool(hp.include_bg_in_dice), float(hp.ce_weight), float(hp.dice_weight))
        return loss, out4[2], out4[0]

    def _step(self, batch, stage):
        x, y = _image_label(batch)
        logits = self(x)
        y = torch.as_tensor(y).to(logits.device)
        loss, macro_dice, _ = self._loss(logits, y)
        self.log(f"{stage}_loss", loss, on_epoch=True, prog_bar=True, sync_dist=True)
        self.log(f"{stage}_macro_dice", macro_dice, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss
