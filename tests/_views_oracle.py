"""The prediction-view fixtures (tests/golden/views_*.npz, make_golden_views.py) and numpy
restatements of what csrc/views.hip computes (test infrastructure; numpy only, importable
without a device): the views of train.py:649-671 in the dtype of the logits given, and the
five-panel strip of train.py:1096-1111 in float64."""
import json
import pathlib
import struct
import zlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
FIXTURES = ("views_k13_d5", "views_ragged", "views_k32_d3", "views_deep", "views_d1")
TIE = 1e-5        # a pixel whose top two fp64 values are closer is a near tie
MAX_TIES = 0.005  # at most this share of the pixels may be left out of a class-map check
_CACHE = {}


def load(name):
    """the fixture as a dict (shared between the tests and left unchanged)"""
    if name not in _CACHE:
        with np.load(GOLDEN / f"{name}.npz") as z:
            d = {k: z[k] for k in z.files}
        d["meta"] = json.loads(str(d["meta"]))
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = d
    return _CACHE[name]


def softmax(row):
    """train.py:611-614 on [K, ...]: max-subtracted exp over the sum in class order + 1e-8"""
    e = np.exp(row - row.max(axis=0, keepdims=True))
    s = e[0].copy()
    for k in range(1, e.shape[0]):
        s += e[k]
    return e / (s + row.dtype.type(1e-8))


def views(logits):
    """logits [B, K, D, H, W] -> center_pred, alpha_center, mip_prob [B, K, H, W], mip_pred,
    in the logits' dtype; argmax takes the first maximum."""
    B, K, D, H, W = logits.shape
    p = np.stack([softmax(logits[:, :, z].swapaxes(0, 1)) for z in range(D)])  # [D, K, B, H, W]
    pc = p[D // 2]
    mip = p.max(axis=0)
    return (pc.argmax(axis=0).astype(np.uint8), pc.max(axis=0), mip.swapaxes(0, 1),
            mip.argmax(axis=0).astype(np.uint8))


def top2_gap(p, axis):
    if p.shape[axis] < 2:
        return np.full(np.delete(p.shape, axis), np.inf)
    t = np.sort(p, axis=axis)
    return np.take(t, -1, axis) - np.take(t, -2, axis)


def comparable(d):
    """(centre mask, mip mask, block mask), each [B, H, W]: the pixels on which a class map
    must equal the reference's -- all of the saturated block, and outside it the pixels whose
    top two fp64 values are at least TIE apart."""
    lg64 = d["logits"].astype(np.float64)
    B, K, D, H, W = lg64.shape
    block = np.zeros((B, H, W), dtype=bool)
    block[:, :, :int(d["block_w"])] = True
    pc = softmax(lg64[:, :, D // 2].swapaxes(0, 1))
    centre_ok = block | (top2_gap(pc, 0) >= TIE)
    mip_ok = block | (top2_gap(d["mip_prob64"], 1) >= TIE)
    return centre_ok, mip_ok, block


def prob_tol(d):
    """max(8 e32, (3 K + 8) 2^-24) for alpha_center and for mip_prob: e32 is the reference's
    own fp32-vs-fp64 error; the floor is K exps and adds of relative 2^-24 each, the max
    subtraction and the division on values <= 1 (the rule of test_r2u_dice_loss_kernel)."""
    floor = (3 * d["meta"]["K"] + 8) * 2.0 ** -24
    return max(8 * float(d["e32_alpha"]), floor), max(8 * float(d["e32_mip"]), floor)


def grey64(img, lo, hi):
    """float64 255 (v - min) / (max - min) before rounding, 0 where max == min; [B, H, W]"""
    img = img.astype(np.float64)
    lo = np.asarray(lo, np.float64)[:, None, None]
    hi = np.asarray(hi, np.float64)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 255.0 * (img - lo) / (hi - lo)
    return np.where(hi == lo, 0.0, g)


def overlay64(center, mip, labels_center, center_pred, mip_pred, alpha_center, table, K):
    """The strip [B, H, 5 W, 3] as unrounded float64 values plus panel 0's unrounded grey:
    grey values rounded first (np.rint), then (1 - a) g + a colour left unrounded, so a
    caller can tell how far a byte is from a rounding boundary."""
    B, H, W = center.shape
    lo_c, hi_c = center.reshape(B, -1).min(1), center.reshape(B, -1).max(1)
    lo_m, hi_m = mip.reshape(B, -1).min(1), mip.reshape(B, -1).max(1)
    g_raw = grey64(center, lo_c, hi_c)
    gc, gm = np.rint(g_raw), np.rint(grey64(mip, lo_m, hi_m))
    tab = table.astype(np.float64)

    def blend(g, cls, a):
        a = np.broadcast_to(np.asarray(a, np.float64), g.shape)[..., None]
        return (1.0 - a) * g[..., None] + a * tab[cls]

    grey3 = np.repeat(gc[..., None], 3, axis=-1)
    if labels_center is None:
        p1 = grey3
    else:
        y = labels_center
        ok = (y >= 0) & (y < K) & (y != 255)
        p1 = np.where(ok[..., None], blend(gc, np.where(ok, y, 0), 0.85), grey3)
    a4 = 0.8 * np.clip(alpha_center.astype(np.float64), 0.35, 1.0)
    panels = [grey3, p1, blend(gc, center_pred, 0.85), blend(gm, mip_pred, 0.85),
              blend(gc, center_pred, a4)]
    return np.concatenate(panels, axis=2), g_raw


def decode_png(path):
    """uint8 [H, W, 3] of an 8-bit RGB PNG: PIL where it is installed, else a zlib parse of
    the unfiltered, non-interlaced files write_png makes"""
    try:
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"))
    except ImportError:
        pass
    raw = pathlib.Path(path).read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0) and tag == b"IEND"
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()  # filter type 0 on every row
    return rows[:, 1:].reshape(h, w, 3)
