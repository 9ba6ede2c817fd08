"""Torch-CPU restatement of sliding-window blending (test infrastructure).

Its own statement of the window starts, the axis weights, the blend and the normaliser,
written from the semantics and not from innovative3D/tiling.py or csrc/tile.hip, in an fp64
and an fp32 mode.  The per-window network outputs are an input: ``tiles`` [n, rd, rh, rw, K]
fp32, channel-last, one per row of the window table.  Imports no other test module."""
import math

import numpy as np
import torch

# name: (volume, roi, overlap, K, starts z / y / x, windows, max cover)
CASES = {
    "overlap_3d": ((12, 24, 28), (8, 16, 16), 0.5, 6, ([0, 4], [0, 8], [0, 8, 12]), 12, 12),
    "registry": ((5, 24, 40), (16, 16, 16), 0.25, 13, ([0], [0, 8], [0, 12, 24]), 6, 4),
    "deep_cover": ((9, 17, 19), (4, 8, 8), 0.75, 32,
                   ([0, 1, 2, 3, 4, 5], [0, 2, 4, 6, 8, 9], [0, 2, 4, 6, 8, 10, 11]), 252, 100),
    "single": ((6, 10, 12), (8, 16, 16), 0.5, 2, ([0], [0], [0]), 1, 1),
}


def starts(n, roi, overlap):
    r = min(roi, n)
    if n == r:
        return [0]
    step = max(1, int(r * (1 - overlap)))
    count = math.ceil((n - r) / step) + 1
    return [min(i * step, n - r) for i in range(count)]


def weights(r, blend, sigma_scale=0.125):
    """fp32 [r] (numpy): the fp64 formula rounded"""
    if blend == "constant":
        return np.ones(r, dtype=np.float32)
    assert blend == "gaussian"
    c, sig = (r - 1) / 2.0, sigma_scale * r
    return np.array([math.exp(-((i - c) ** 2) / (2.0 * sig * sig)) for i in range(r)],
                    dtype=np.float64).astype(np.float32)


def flip_sets(mirror_axes):
    """the flip bits of every subset of the axes, the empty subset first"""
    axes = sorted(set(mirror_axes))
    return [sum(1 << axes[j] for j in range(len(axes)) if m >> j & 1)
            for m in range(1 << len(axes))]


def table(vol, roi, overlap, mirror_axes=()):
    r = [min(a, b) for a, b in zip(roi, vol)]
    per_axis = [starts(n, ri, overlap) for n, ri in zip(vol, r)]
    return [(z, y, x, f) for f in flip_sets(mirror_axes) for z in per_axis[0]
            for y in per_axis[1] for x in per_axis[2]]


def flip_dims(bits, first=0):
    """the tensor dims of flip bits 1 = D, 2 = H, 4 = W when D is dim ``first``"""
    return [first + a for a in range(3) if bits >> a & 1]


def blend(tiles, tab, vol, blend_kind, blend_of, dtype, sigma_scale=0.125):
    """acc [D, H, W, K] in ``dtype``: sum over the table rows, in order, of w * s mirrored back,
    s the tile or its softmax over K computed in ``dtype``; w = (wz wy) wx of the fp32 axis
    weights, multiplied in ``dtype``."""
    n, rd, rh, rw, K = tiles.shape
    assert n == len(tab)
    wz, wy, wx = (torch.from_numpy(weights(r, blend_kind, sigma_scale)).to(dtype)
                  for r in (rd, rh, rw))
    w = ((wz[:, None, None] * wy[None, :, None]) * wx[None, None, :])[..., None]
    acc = torch.zeros(tuple(vol) + (K,), dtype=dtype)
    for i, (z0, y0, x0, f) in enumerate(tab):
        s = tiles[i].to(dtype)
        if blend_of == "probs":
            s = torch.softmax(s, dim=-1)
        else:
            assert blend_of == "logits"
        t = w * s
        if f:
            t = torch.flip(t, flip_dims(f))
        acc[z0:z0 + rd, y0:y0 + rh, x0:x0 + rw] += t
    return acc


def norms(vol, roi, overlap, blend_kind, sigma_scale=0.125):
    """fp32 (nz, ny, nx) (numpy): the fp64 sums of the fp32 axis weights, rounded"""
    out = []
    for n, ri in zip(vol, [min(a, b) for a, b in zip(roi, vol)]):
        w = weights(ri, blend_kind, sigma_scale).astype(np.float64)
        s = np.zeros(n, dtype=np.float64)
        for st in starts(n, ri, overlap):
            s[st:st + ri] += w
        out.append(s.astype(np.float32))
    return out


def scores(acc, nvec, flips):
    """acc / (flips nz[z] ny[y] nx[x]) in acc's dtype"""
    nz, ny, nx = (torch.from_numpy(v).to(acc.dtype) for v in nvec)
    norm = ((float(flips) * nz)[:, None, None] * ny[None, :, None]) * nx[None, None, :]
    return acc / norm[..., None]


def case_tiles(name, seed=0):
    """the kernel cases' synthetic window outputs 3 randn [n, rd, rh, rw, K] fp32, and labels
    [D, H, W] int64 with 5 % 255 and a few K + 3"""
    vol, roi, overlap, K, _st, n, _cover = CASES[name]
    r = [min(a, b) for a, b in zip(roi, vol)]
    g = torch.Generator().manual_seed(seed)
    tiles = 3.0 * torch.randn(n, *r, K, generator=g)
    labels = torch.randint(0, K, tuple(vol), generator=g)
    labels[torch.rand(tuple(vol), generator=g) < 0.05] = 255
    labels.view(-1)[::97] = K + 3
    return tiles, labels


def sum_bound(cover, max_abs, K=0):
    """What an fp32 blend may differ from the fp64 one by, per normalised score: a sum of
    ``cover`` products of two fp32-rounded factors, each add rounded once, then one division
    -- (cover + 3) half-ulps of the largest |term| sum, which is at most max|s| after the
    division; the softmax adds its own K adds, an exp and a division per entry."""
    return (cover + 3 + (K + 8 if K else 0)) * 2.0 ** -24 * max_abs
