"""Test oracle of the SPCT core with spatial attention and gated skips (test infrastructure).

The forward of oracle.spff_oracle.forward with the two extra steps of the reference's
UNet3D_SpectralCore (models.py:434-446 SpatialAttention3D after every encoder stage's
Spectral-SE and Channel-SE; models.py:627-645 AttentionGate3d on the three skips, called
with the up-conv output first, so the gate multiplies the up-conv output).  Blocks, SE,
pools, _cat and the loss are the oracle's own, by import.

``as_oracle_forward(spatial, skip_gate)`` installs this forward as ``O.forward`` for the
duration of a ``with`` block, so ``O.fwd_bwd``, ``_kink.resolve_kinks`` and
``_kink.forced_branches`` run it unchanged.  The new branch decisions have hooks in the
style of tests/_kink.forced_branches: ``channel_max`` (the ``sa`` argmax index) and
``gate_relu`` (the gates' ReLU signs), forced by ``forced_spatial``.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import spff_oracle as O

STAGES = ("enc1", "enc2", "enc3", "bott")
GATES = ("g3", "g2", "g1")


def channel_max(z, stage):
    """max over the channels of z [B, C, D, H, W] -> [B, 1, D, H, W] (hook: the argmax)."""
    return z.max(dim=1, keepdim=True)[0]


def gate_relu(h, gate):
    """ReLU of a gate's hidden row [B, I, D, H, W] (hook: the sign pattern)."""
    return F.relu(h)


def spatial_attention(P, pre, z, stage):
    m = torch.cat([z.mean(dim=1, keepdim=True), channel_max(z, stage)], dim=1)
    return z * torch.sigmoid(F.conv3d(m, P[pre + ".conv.weight"], None, padding=(1, 3, 3)))


def attention_gate(P, pre, d, e):
    """AttentionGate.forward(x_skip = d, g = e): d * sigmoid(psi(relu(W_x d + W_g e)))."""
    h = F.conv3d(d, P[pre + ".W_x.weight"], P[pre + ".W_x.bias"]) + \
        F.conv3d(e, P[pre + ".W_g.weight"], P[pre + ".W_g.bias"])
    att = gate_relu(h, pre)
    return d * torch.sigmoid(F.conv3d(att, P[pre + ".psi.weight"], P[pre + ".psi.bias"]))


def forward(P, x, cfg, spatial=False, skip_gate=False):
    up = lambda t, n: F.conv_transpose3d(t, P[n + ".weight"], P[n + ".bias"], stride=(1, 2, 2))  # noqa: E731

    def post(t, i):
        t = O._post(P, t, i, cfg)
        return spatial_attention(P, f"sa.{i}", t, STAGES[i]) if spatial else t

    def skip(d, e, g):
        return attention_gate(P, g, d, e) if skip_gate else e

    e1 = post(O.novel_block(P, "enc1", x, cfg), 0)
    e2 = post(O.novel_block(P, "enc2", O.maxpool(e1), cfg), 1)
    e3 = post(O.novel_block(P, "enc3", O.maxpool(e2), cfg), 2)
    b = post(O.novel_block(P, "bott", O.maxpool(e3), cfg), 3)
    d3 = up(b, "up3")
    d3 = O.novel_block(P, "dec3", O._cat(d3, skip(d3, e3, "g3")), cfg)
    d2 = up(d3, "up2")
    d2 = O.novel_block(P, "dec2", O._cat(d2, skip(d2, e2, "g2")), cfg)
    d1 = up(d2, "up1")
    d1 = O.novel_block(P, "dec1", O._cat(d1, skip(d1, e1, "g1")), cfg)
    return F.conv3d(d1, P["out.weight"], P["out.bias"])


def param_shapes(cfg, D=None, prefix="", spatial=False, skip_gate=False):
    """State-dict keys / shapes in the reference's registration order: the oracle's, then
    sa.0..3, g3, g2, g1 (models.py:676-682)."""
    out = list(O.param_shapes(cfg, D=D, prefix=prefix).items())
    f = cfg.base
    if spatial:
        out += [(f"{prefix}sa.{i}.conv.weight", (1, 2, 3, 7, 7)) for i in range(4)]
    if skip_gate:
        for g, C, I in (("g3", 4 * f, 2 * f), ("g2", 2 * f, f), ("g1", f, f // 2)):
            out += [(f"{prefix}{g}.W_x.weight", (I, C, 1, 1, 1)), (f"{prefix}{g}.W_x.bias", (I,)),
                    (f"{prefix}{g}.W_g.weight", (I, C, 1, 1, 1)), (f"{prefix}{g}.W_g.bias", (I,)),
                    (f"{prefix}{g}.psi.weight", (1, I, 1, 1, 1)), (f"{prefix}{g}.psi.bias", (1,))]
    return OrderedDict(out)


class as_oracle_forward:
    """``with as_oracle_forward(spatial, skip_gate):`` O.forward is this module's forward."""

    def __init__(self, spatial, skip_gate):
        self.kw = dict(spatial=bool(spatial), skip_gate=bool(skip_gate))

    def __enter__(self):
        self._orig = O.forward
        O.forward = lambda P, x, cfg: forward(P, x, cfg, **self.kw)
        return self

    def __exit__(self, *exc):
        O.forward = self._orig
        return False


class forced_spatial:
    """The ``sa`` channel max takes the given argmax index (``masks["enc1.sa.idx"]``
    [B, D, H, W], likewise enc2, enc3, bott) and the gates' ReLUs the given sign pattern
    (``masks["g3.att"]`` bool [B, I, D, H, W], likewise g2, g1); keys that are absent keep
    the oracle's own decision.  A run on one sample of the batch the masks were taken from
    (the per-sample gradient sums of tests/_spff_checks.oracle_grads_st, which walks the
    samples in order) takes that sample's slice: the n-th one-sample call of a key reads
    sample n mod B."""

    def __init__(self, masks):
        self.masks = masks
        self._seen = {}

    def _mask(self, key, like):
        m = self.masks.get(key)
        if m is not None and m.shape[0] != like.shape[0]:
            assert like.shape[0] == 1, (key, m.shape, like.shape)
            b = self._seen.get(key, 0)
            self._seen[key] = b + 1
            m = m[b % m.shape[0]:b % m.shape[0] + 1]
        return m

    def _max(self, z, stage):
        m = self._mask(stage + ".sa.idx", z)
        if m is None:
            return self._orig[0](z, stage)
        return z.gather(1, m.to(z.device).long().unsqueeze(1))

    def _relu(self, h, gate):
        m = self._mask(gate + ".att", h)
        if m is None:
            return self._orig[1](h, gate)
        return torch.where(m.to(h.device), h, torch.zeros_like(h))

    def __enter__(self):
        g = globals()
        self._orig = g["channel_max"], g["gate_relu"]
        g["channel_max"], g["gate_relu"] = self._max, self._relu
        return self

    def __exit__(self, *exc):
        g = globals()
        g["channel_max"], g["gate_relu"] = self._orig
        return False
