"""UNETR oracle: MONAI 1.5.2's ``monai.networks.nets.UNETR`` restated in plain torch, plus
the reference's LitUNETR_Published wrapper (models.py:1006-1061: pad, resample, crop, loss)
as functions, in whatever dtype the parameters have (fp64 for the tests).

PARITY UNPINNED.  MONAI cannot be imported here, so EVERYTHING this file says about MONAI is
an assumption that nobody could check against MONAI itself:

* wrapper arguments: UNETR_Published filters its keyword arguments by MONAI's signature;
  MONAI 1.5 has no ``pos_embed`` argument, so ``proj_type="conv"`` applies and the position
  embedding is learnable;
* ViT patch embedding: Conv3d(in, hidden, 16, stride 16) with bias, flattened to [B, n, hidden]
  in D, H, W order, plus position_embeddings [1, n, hidden];
* twelve blocks ``x = x + out_proj(SA(LN1 x))``, ``x = x + W2 gelu(W1 LN2 x)``; LayerNorm eps
  1e-5; qkv = Linear(hidden, 3 hidden) without bias, split as (qkv, head, d); scale d^-0.5;
  softmax over all n keys; out_proj with bias; exact (erf) GELU; the final vit.norm after
  the twelve blocks; hidden_states_out[i] = block i's output;
* decoder: encoder1 = UnetrBasicBlock(in -> f) on the input; encoder2 / 3 / 4 =
  UnetrPrUpBlock(hidden -> 2f / 4f / 8f, num_layer 2 / 1 / 0) on proj_feat of hidden states
  3 / 6 / 9 (a 2x2x2 stride-2 transposed conv without bias, then per layer another such
  transposed conv and a UnetResBlock); decoder5 .. decoder2 = UnetrUpBlock (transposed conv,
  cat[up, skip], UnetResBlock), decoder5 on proj_feat of the normed output; out = 1x1x1 conv
  with bias; InstanceNorm without affine, LeakyReLU slope 0.01;
* parameter names and registration order (a module's own parameters before its children's),
  including norm_cross_attn and cross_attn.* that MONAI >= 1.4 registers in every block and
  never uses on this path.

The fixtures tests/golden/unetr_*.npz run the REFERENCE's LitUNETR_Published around this
module (tests/golden/make_golden_unetr.py), so they pin the reference's pad / resample /
crop / loss / gradient flow, not the body.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

# kink-consistent runs: "<residual block>.act1" / ".act2" -> bool sign mask [B, C, D, H, W]
ACT_MASKS: Optional[Dict[str, torch.Tensor]] = None


def _lrelu(name, t):
    if ACT_MASKS is None:
        return F.leaky_relu(t, 0.01)
    return torch.where(ACT_MASKS[name].to(t.device), t, 0.01 * t)


class _Conv(nn.Module):
    """MONAI Convolution(conv_only=True): the conv sits under ``.conv``."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def forward(self, x):
        return self.conv(x)


def _transp(ci, co):
    return _Conv(nn.ConvTranspose3d(ci, co, 2, stride=2, bias=False))


class _ResBlock(nn.Module):
    """MONAI UnetResBlock with InstanceNorm3d (no affine) and LeakyReLU(0.01)."""

    def __init__(self, ci, co):
        super().__init__()
        self.conv1 = _Conv(nn.Conv3d(ci, co, 3, padding=1, bias=False))
        self.conv2 = _Conv(nn.Conv3d(co, co, 3, padding=1, bias=False))
        if ci != co:
            self.conv3 = _Conv(nn.Conv3d(ci, co, 1, bias=False))
        self.tag = ""

    def forward(self, x):
        y = _lrelu(self.tag + ".act1", F.instance_norm(self.conv1(x), eps=1e-5))
        y = F.instance_norm(self.conv2(y), eps=1e-5)
        r = F.instance_norm(self.conv3(x), eps=1e-5) if hasattr(self, "conv3") else x
        return _lrelu(self.tag + ".act2", y + r)


class _Holder(nn.Module):
    pass


class _Block(nn.Module):
    def __init__(self, hidden, mlp_dim, heads):
        super().__init__()
        self.heads = heads
        self.mlp = _Holder()
        self.mlp.linear1 = nn.Linear(hidden, mlp_dim)
        self.mlp.linear2 = nn.Linear(mlp_dim, hidden)
        self.norm1 = nn.LayerNorm(hidden)
        self.attn = _Holder()
        self.attn.out_proj = nn.Linear(hidden, hidden)
        self.attn.qkv = nn.Linear(hidden, 3 * hidden, bias=False)
        self.norm2 = nn.LayerNorm(hidden)
        # registered by MONAI >= 1.4, unused without with_cross_attention
        self.norm_cross_attn = nn.LayerNorm(hidden)
        self.cross_attn = _Holder()
        self.cross_attn.out_proj = nn.Linear(hidden, hidden)
        self.cross_attn.to_q = nn.Linear(hidden, hidden, bias=False)
        self.cross_attn.to_k = nn.Linear(hidden, hidden, bias=False)
        self.cross_attn.to_v = nn.Linear(hidden, hidden, bias=False)

    def forward(self, x):
        B, n, C = x.shape
        hd = C // self.heads
        qkv = self.attn.qkv(self.norm1(x)).reshape(B, n, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5, dim=-1)
        o = (att @ qkv[2]).transpose(1, 2).reshape(B, n, C)
        x = x + self.attn.out_proj(o)
        return x + self.mlp.linear2(F.gelu(self.mlp.linear1(self.norm2(x))))


class _PrUp(nn.Module):
    def __init__(self, hidden, co, num_layer):
        super().__init__()
        self.transp_conv_init = _transp(hidden, co)
        self.blocks = nn.ModuleList([nn.Sequential(_transp(co, co), _ResBlock(co, co))
                                     for _ in range(num_layer)])

    def forward(self, x):
        x = self.transp_conv_init(x)
        for b in self.blocks:
            x = b(x)
        return x


class _Up(nn.Module):
    def __init__(self, ci, co):
        super().__init__()
        self.transp_conv = _transp(ci, co)
        self.conv_block = _ResBlock(2 * co, co)

    def forward(self, x, skip):
        return self.conv_block(torch.cat([self.transp_conv(x), skip], dim=1))


class UNETR(nn.Module):
    """MONAI 1.5.2's constructor signature and state-dict keys."""

    def __init__(self, in_channels, out_channels, img_size, feature_size=16, hidden_size=768,
                 mlp_dim=3072, num_heads=12, proj_type="conv", norm_name="instance",
                 conv_block=True, res_block=True, dropout_rate=0.0, spatial_dims=3,
                 qkv_bias=False, save_attn=False):
        super().__init__()
        assert proj_type == "conv" and conv_block and res_block and not qkv_bias
        assert spatial_dims == 3 and dropout_rate == 0.0 and norm_name == "instance"
        if isinstance(img_size, int):
            img_size = (img_size,) * 3
        if hidden_size % num_heads:
            raise ValueError("hidden_size should be divisible by num_heads.")
        self.feat = tuple(int(v) // 16 for v in img_size)
        self.hidden = hidden_size
        n = self.feat[0] * self.feat[1] * self.feat[2]
        f = feature_size
        self.vit = _Holder()
        self.vit.patch_embedding = _Holder()
        self.vit.patch_embedding.position_embeddings = nn.Parameter(torch.zeros(1, n, hidden_size))
        nn.init.trunc_normal_(self.vit.patch_embedding.position_embeddings, std=0.02)
        self.vit.patch_embedding.patch_embeddings = nn.Conv3d(in_channels, hidden_size, 16, stride=16)
        self.vit.blocks = nn.ModuleList([_Block(hidden_size, mlp_dim, num_heads) for _ in range(12)])
        self.vit.norm = nn.LayerNorm(hidden_size)
        self.encoder1 = _Holder()
        self.encoder1.layer = _ResBlock(in_channels, f)
        self.encoder2 = _PrUp(hidden_size, 2 * f, 2)
        self.encoder3 = _PrUp(hidden_size, 4 * f, 1)
        self.encoder4 = _PrUp(hidden_size, 8 * f, 0)
        self.decoder5 = _Up(hidden_size, 8 * f)
        self.decoder4 = _Up(8 * f, 4 * f)
        self.decoder3 = _Up(4 * f, 2 * f)
        self.decoder2 = _Up(2 * f, f)
        self.out = _Holder()
        self.out.conv = _Conv(nn.Conv3d(f, out_channels, 1, bias=True))
        for name, m in self.named_modules():
            if isinstance(m, _ResBlock):
                m.tag = name

    def proj_feat(self, x):
        B = x.shape[0]
        return x.view(B, *self.feat, self.hidden).permute(0, 4, 1, 2, 3).contiguous()

    def forward(self, x_in):
        pe = self.vit.patch_embedding
        x = pe.patch_embeddings(x_in).flatten(2).transpose(-1, -2) + pe.position_embeddings
        hs = []
        for blk in self.vit.blocks:
            x = blk(x)
            hs.append(x)
        x = self.vit.norm(x)
        enc1 = self.encoder1.layer(x_in)
        enc2 = self.encoder2(self.proj_feat(hs[3]))
        enc3 = self.encoder3(self.proj_feat(hs[6]))
        enc4 = self.encoder4(self.proj_feat(hs[9]))
        dec3 = self.decoder5(self.proj_feat(x), enc4)
        dec2 = self.decoder4(dec3, enc3)
        dec1 = self.decoder3(dec2, enc2)
        return self.out.conv(self.decoder2(dec1, enc1))


def used_keys(state_keys):
    """The state-dict keys the forward uses (MONAI's unused cross-attention holders out)."""
    return [k for k in state_keys if "cross_attn" not in k]


# ------------------------------------------------- the reference's Lit wrapper --
def pad16(x):
    """_pad_to_mult16_3d: replicate, centred, to multiples of 16."""
    D, H, W = x.shape[-3:]
    pd, ph, pw = (-D) % 16, (-H) % 16, (-W) % 16
    pads = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2, pd // 2, pd - pd // 2)
    return (F.pad(x, pads, mode="replicate") if any(pads) else x), (D, H, W)


def crop(y, orig):
    D, H, W = orig
    Dp, Hp, Wp = y.shape[-3:]
    d0, h0, w0 = (Dp - D) // 2, (Hp - H) // 2, (Wp - W) // 2
    return y[..., d0:d0 + D, h0:h0 + H, w0:w0 + W]


def lin_axis(n_in, n_out, dtype):
    """ATen upsample_trilinear3d, align_corners=False, size given, one axis: (i0, i1, l0, l1).
    src = max(0, (dst + 0.5) * in / out - 0.5); the upper neighbour is clamped."""
    o = torch.arange(n_out, dtype=dtype)
    src = ((o + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.to(dtype)
    if n_in == n_out:
        l1 = torch.zeros_like(l1)
    return i0, i1, 1 - l1, l1


def resize3d(x, size):
    """The resample restated with index_select (differentiable): equals F.interpolate
    (trilinear, align_corners=False) and its autograd."""
    for ax, n_out in zip((2, 3, 4), size):
        i0, i1, l0, l1 = lin_axis(x.shape[ax], int(n_out), x.dtype)
        shp = [1] * x.ndim
        shp[ax] = -1
        x = x.index_select(ax, i0) * l0.view(shp) + x.index_select(ax, i1) * l1.view(shp)
    return x


def lit_forward(net, x, img_size):
    """LitUNETR_Published.forward."""
    if isinstance(x, (list, tuple)):
        x = x[0]
    if x.ndim == 4:
        x = x.unsqueeze(1)
    xp, orig = pad16(x)
    target = tuple(int(v) for v in img_size)
    xr = resize3d(xp, target) if tuple(xp.shape[2:]) != target else xp
    yr = net(xr)
    yp = resize3d(yr, xp.shape[2:]) if tuple(yr.shape[2:]) != tuple(xp.shape[2:]) else yr
    return crop(yp, orig)


def lit_loss(logits, labels, ignore_index=255, include_bg=False, ce_weight=0.5, eps=1e-6):
    """LitUNETR_Published._loss (= LitSwinUNETR_Published._loss): returns (loss, dice_loss, ce)."""
    C = logits.shape[1]
    probs = torch.softmax(logits, dim=1)
    lab = labels
    if ignore_index is not None:
        mask = (labels != ignore_index).unsqueeze(1).to(logits.dtype)
        lab = torch.where(labels == ignore_index, torch.zeros_like(labels), labels)
        probs = probs * mask
    onehot = F.one_hot(lab.clamp_min(0), num_classes=C).permute(0, 4, 1, 2, 3).to(logits.dtype)
    s = 0 if include_bg else 1
    p, g = probs[:, s:], onehot[:, s:]
    inter = (p * g).sum(dim=(2, 3, 4))
    den = p.sum(dim=(2, 3, 4)) + g.sum(dim=(2, 3, 4)) + eps
    dice = 1.0 - (2.0 * inter / den).mean()
    ce = F.cross_entropy(logits, labels, ignore_index=ignore_index if ignore_index is not None
                         else -100)
    return (1.0 - ce_weight) * dice + ce_weight * ce, dice, ce


def build(meta, state, dtype=torch.float64):
    """The oracle module of a fixture's ``meta`` with the state dict ``state`` (numpy, keys
    with or without the Lit module's "net.net." prefix)."""
    net = UNETR(in_channels=meta["in_ch"], out_channels=meta["K"], img_size=tuple(meta["img"]),
                feature_size=meta["feature_size"], hidden_size=meta["hidden"],
                mlp_dim=meta["mlp_dim"], num_heads=meta["heads"])
    sd = {(k[len("net.net."):] if k.startswith("net.net.") else k): torch.as_tensor(v)
          for k, v in state.items()}
    net.load_state_dict(sd, strict=True)
    return net.to(dtype)


def fwd_bwd(net, x, labels, meta):
    """logits, loss and the gradients of the used parameters, in the module's dtype."""
    net.zero_grad(set_to_none=True)
    dt = next(net.parameters()).dtype
    logits = lit_forward(net, x.to(dt), meta["img"])
    loss, _dice, _ce = lit_loss(logits, labels, meta.get("ignore_index", 255),
                                meta.get("include_bg", False), meta.get("ce_weight", 0.5))
    loss.backward()
    grads = {k: p.grad.detach().double() for k, p in net.named_parameters() if p.grad is not None}
    return logits.detach(), loss.detach(), grads


def lr_at(t, lr, warmup_iters, total_iters):
    """on_train_batch_start's learning rate at iteration t (models.py:1072-1078)."""
    if t < warmup_iters:
        return lr * float(t + 1) / max(1, warmup_iters)
    prog = (t - warmup_iters) / max(1, max(1, total_iters) - warmup_iters)
    return 0.5 * lr * (1.0 + math.cos(math.pi * prog))
