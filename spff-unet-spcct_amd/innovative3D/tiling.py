"""Host side of sliding-window inference: where the windows lie, what they
weigh and what the weights sum to.  numpy only, importable without a device; the kernels
are csrc/tile.hip and the driver is helpers.predict_tiled.

Along one axis of length ``n``, for a requested window ``roi`` and ``overlap`` in [0, 1):
``r = min(roi, n)``, ``step = max(1, int(r * (1 - overlap)))``,
``count = ceil((n - r) / step) + 1`` and ``start_i = min(i * step, n - r)``: the starts are
distinct and the last window ends at ``n``.  The 3-D windows are the Cartesian product,
z-major, then y, then x.  The weight of a window voxel is the product of three axis weights,
so the sum of the weights over the windows is a product of three axis sums: no weight-sum
volume exists."""
from __future__ import annotations

import itertools
from typing import List, Sequence, Tuple

import numpy as np

MAX_WINDOWS = 64  # SPFF_TILE_MAX_WINDOWS: windows per engine call
BLENDS = ("gaussian", "constant")


def _check_overlap(overlap: float) -> float:
    overlap = float(overlap)
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"overlap must lie in [0, 1), got {overlap}")
    return overlap


def window_starts(n: int, roi: int, overlap: float) -> List[int]:
    """The window starts along an axis of length ``n``."""
    n, roi = int(n), int(roi)
    if n < 1 or roi < 1:
        raise ValueError(f"axis length {n} and window {roi} must be at least 1")
    overlap = _check_overlap(overlap)
    r = min(roi, n)
    if n == r:
        return [0]
    step = max(1, int(r * (1 - overlap)))
    count = -(-(n - r) // step) + 1
    return [min(i * step, n - r) for i in range(count)]


def clamp_roi(vol: Sequence[int], roi: Sequence[int]) -> Tuple[int, int, int]:
    """The window extents the volume allows: min(roi, volume) per axis."""
    if len(vol) != 3 or len(roi) != 3:
        raise ValueError(f"expected three extents, got volume {tuple(vol)} and roi {tuple(roi)}")
    return tuple(min(int(r), int(n)) for r, n in zip(roi, vol))


def axis_weights(r: int, blend: str = "gaussian", sigma_scale: float = 0.125) -> np.ndarray:
    """fp32 [r]: ``gaussian`` exp(-(i - (r - 1) / 2)^2 / (2 (sigma_scale r)^2)), computed in
    fp64 and rounded; ``constant`` ones.  Symmetric bit for bit."""
    r = int(r)
    if r < 1:
        raise ValueError(f"window extent {r} below 1")
    if blend == "constant":
        return np.ones(r, dtype=np.float32)
    if blend != "gaussian":
        raise ValueError(f"blend={blend!r}: expected one of {BLENDS}")
    sigma = float(sigma_scale) * r
    if not sigma > 0.0:
        raise ValueError(f"sigma_scale must be positive, got {sigma_scale}")
    half = (r + 1) // 2  # one half is computed, the other mirrors it
    d = np.arange(half, dtype=np.float64) - (r - 1) / 2.0
    w = np.empty(r, dtype=np.float64)
    w[:half] = np.exp(-(d * d) / (2.0 * sigma * sigma))
    w[r - half:] = w[:half][::-1]
    return w.astype(np.float32)


def flip_passes(mirror_axes: Sequence[int]) -> List[int]:
    """The flip bits (1 = D, 2 = H, 4 = W) of every subset of ``mirror_axes``, the empty
    subset first."""
    axes = sorted({int(a) for a in mirror_axes})
    if any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"mirror_axes {tuple(mirror_axes)}: a subset of (0, 1, 2) = (D, H, W)")
    return [sum(1 << axes[j] for j in range(len(axes)) if m >> j & 1)
            for m in range(1 << len(axes))]


def window_table(vol: Sequence[int], roi: Sequence[int], overlap: float = 0.5,
                 mirror_axes: Sequence[int] = ()) -> np.ndarray:
    """int32 [n][4] = z0, y0, x0, flip bits: one pass over all windows (z-major, then y, then
    x) per subset of ``mirror_axes``, the unflipped pass first."""
    r = clamp_roi(vol, roi)
    starts = [window_starts(n, ri, overlap) for n, ri in zip(vol, r)]
    rows = [(z, y, x, f) for f in flip_passes(mirror_axes)
            for z, y, x in itertools.product(*starts)]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def norm_vectors(vol: Sequence[int], roi: Sequence[int], overlap: float = 0.5,
                 blend: str = "gaussian", sigma_scale: float = 0.125, dtype=np.float32):
    """(nz, ny, nx): per axis the sum of the fp32 axis weights over the starts that cover each
    position, summed in fp64 and rounded to ``dtype``.  The weight sum of one pass over the
    windows at voxel (z, y, x) is nz[z] ny[y] nx[x]; every flip pass adds the same."""
    r = clamp_roi(vol, roi)
    out = []
    for n, ri in zip(vol, r):
        w = axis_weights(ri, blend, sigma_scale).astype(np.float64)
        s = np.zeros(int(n), dtype=np.float64)
        for st in window_starts(n, ri, overlap):
            s[st:st + ri] += w
        out.append(s.astype(dtype))
    return tuple(out)


def batches(n: int, size: int) -> List[Tuple[int, int]]:
    """[start, stop) ranges of at most ``size`` consecutive table rows"""
    size = int(size)
    if not 1 <= size <= MAX_WINDOWS:
        raise ValueError(f"window_batch must be 1..{MAX_WINDOWS}, got {size}")
    return [(i, min(i + size, n)) for i in range(0, n, size)]


def max_cover(vol: Sequence[int], roi: Sequence[int], overlap: float) -> int:
    """The largest number of windows of one pass that cover a voxel."""
    r = clamp_roi(vol, roi)
    cover = 1
    for n, ri in zip(vol, r):
        c = np.zeros(int(n), dtype=np.int64)
        for st in window_starts(n, ri, overlap):
            c[st:st + ri] += 1
        cover *= int(c.max())
    return cover


__all__ = ["MAX_WINDOWS", "BLENDS", "window_starts", "clamp_roi", "axis_weights", "flip_passes",
           "window_table", "norm_vectors", "batches", "max_cover"]
