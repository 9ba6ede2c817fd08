"""Sliding-window inference without a device: the window geometry of innovative3D/tiling.py
against the lists of DESIGN §8.3 and the oracle's own restatement, the separable normaliser
against a brute-force weight sum, the host refusals of the three spff_tile_* entries, and the
oracle's fp32 mode against its fp64 one."""
import ctypes

import numpy as np
import pytest
import torch

import _tile_oracle as TO
from innovative3D import _engine as E
from innovative3D import tiling as T

SPFF_EINVAL, SPFF_ESHAPE = -1, -3


@pytest.mark.parametrize("name", list(TO.CASES))
def test_window_starts_and_table(name):
    vol, roi, overlap, _K, want, n, cover = TO.CASES[name]
    got = [T.window_starts(a, r, overlap) for a, r in zip(vol, roi)]
    assert got == list(want)
    r = T.clamp_roi(vol, roi)
    for s, a, ri in zip(got, vol, r):
        assert len(set(s)) == len(s) and s[-1] + ri == a  # distinct, the last ends at n
    tab = T.window_table(vol, roi, overlap)
    assert tab.dtype == np.int32 and tab.shape == (n, 4)
    assert [tuple(int(v) for v in row) for row in tab] == TO.table(vol, roi, overlap)
    assert T.max_cover(vol, roi, overlap) == cover


def test_window_starts_edges():
    assert T.window_starts(7, 7, 0.9) == [0] and T.window_starts(3, 9, 0.0) == [0]
    assert T.window_starts(10, 4, 0.0) == [0, 4, 6]
    assert T.window_starts(5, 2, 0.99) == [0, 1, 2, 3]  # the step never falls below 1
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            T.window_starts(8, 4, bad)
    with pytest.raises(ValueError):
        T.window_starts(0, 4, 0.5)
    with pytest.raises(ValueError):
        T.batches(5, 65)


def test_mirror_passes_run_outside_the_windows():
    vol, roi, overlap = (12, 24, 28), (8, 16, 16), 0.5
    assert T.flip_passes(()) == [0] and T.flip_passes((2,)) == [0, 4]
    assert T.flip_passes((1, 0)) == [0, 1, 2, 3] and T.flip_passes((0, 1, 2)) == list(range(8))
    one = T.window_table(vol, roi, overlap)
    tab = T.window_table(vol, roi, overlap, (0, 2))
    assert tab.shape == (4 * len(one), 4)
    for p, bits in enumerate((0, 1, 4, 5)):  # the empty subset first, windows inside
        blk = tab[p * len(one):(p + 1) * len(one)]
        assert np.array_equal(blk[:, :3], one[:, :3]) and (blk[:, 3] == bits).all()
    assert [tuple(int(v) for v in row) for row in tab] == TO.table(vol, roi, overlap, (0, 2))
    with pytest.raises(ValueError):
        T.flip_passes((3,))


@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 8, 16, 17, 128])
def test_axis_weights_are_symmetric_bit_for_bit(r):
    for blend in T.BLENDS:
        w = T.axis_weights(r, blend)
        assert w.dtype == np.float32 and w.shape == (r,)
        assert np.array_equal(w.view(np.uint32), w[::-1].view(np.uint32))
        assert np.array_equal(w.view(np.uint32), TO.weights(r, blend).view(np.uint32))
        assert (w > 0).all() and w.max() <= 1.0
    assert (T.axis_weights(r, "constant") == 1).all()
    with pytest.raises(ValueError):
        T.axis_weights(r, "cosine")


@pytest.mark.parametrize("blend", T.BLENDS)
@pytest.mark.parametrize("name", list(TO.CASES))
def test_norm_vectors_against_the_brute_force_sum(name, blend):
    vol, roi, overlap, _K, _st, _n, _cover = TO.CASES[name]
    mirror = (0, 2)
    r = T.clamp_roi(vol, roi)
    wz, wy, wx = (T.axis_weights(ri, blend).astype(np.float64) for ri in r)
    w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    brute = np.zeros(vol, dtype=np.float64)
    for z, y, x, _f in T.window_table(vol, roi, overlap, mirror):  # (the weight is symmetric)
        brute[z:z + r[0], y:y + r[1], x:x + r[2]] += w3
    nz, ny, nx = T.norm_vectors(vol, roi, overlap, blend, dtype=np.float64)
    flips = len(T.flip_passes(mirror))
    sep = flips * nz[:, None, None] * ny[None, :, None] * nx[None, None, :]
    assert brute.min() > 0
    assert float(np.abs(sep / brute - 1).max()) <= 1e-12
    for a, b, c in zip(T.norm_vectors(vol, roi, overlap, blend), (nz, ny, nx),
                       TO.norms(vol, roi, overlap, blend)):
        assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32))
        assert np.array_equal(a, c)


def _refusal_args():
    """host buffers stand in for device memory: every refusal comes before any device call"""
    buf = (ctypes.c_float * 64)()
    i64 = (ctypes.c_int64 * 64)()
    return ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(i64, ctypes.c_void_p)


def _tab(*rows):
    return (ctypes.c_int32 * (4 * len(rows)))(*[v for r in rows for v in r])


def _last_error():
    return E.lib().spff_last_error().decode()


def test_tile_gather_refusals():
    L = E.lib()
    p, _ = _refusal_args()
    ok = _tab((0, 0, 0, 0))

    def call(x=p, C=1, vol=(4, 4, 4), tab=ok, n=1, roi=(2, 2, 2), out=p):
        return L.spff_tile_gather(x, C, *vol, tab, n, *roi, out, None)
    assert call(x=None) == SPFF_EINVAL and "null" in _last_error()
    assert call(out=None) == SPFF_EINVAL
    assert call(tab=None) == SPFF_EINVAL
    assert call(n=0) == SPFF_EINVAL and call(n=65) == SPFF_EINVAL
    assert "1..64" in _last_error()
    assert call(tab=_tab((0, 0, 0, 8))) == SPFF_EINVAL and "flip" in _last_error()
    assert call(tab=_tab((0, 0, 0, -1))) == SPFF_EINVAL
    assert call(roi=(5, 2, 2)) == SPFF_ESHAPE and "larger" in _last_error()
    assert call(tab=_tab((3, 0, 0, 0))) == SPFF_ESHAPE and "inside" in _last_error()
    assert call(tab=_tab((0, -1, 0, 0))) == SPFF_ESHAPE
    assert call(tab=_tab((0, 0, 0, 0), (0, 0, 3, 7)), n=2) == SPFF_ESHAPE


def test_tile_accumulate_refusals():
    L = E.lib()
    p, _ = _refusal_args()
    ok = _tab((0, 0, 0, 0))

    def call(tiles=p, tab=ok, n=1, roi=(2, 2, 2), K=4, vol=(4, 4, 4), w=(p, p, p), acc=p):
        return L.spff_tile_accumulate(tiles, tab, n, *roi, K, *vol, *w, 0, acc, None)
    assert call(K=1) == SPFF_EINVAL and call(K=33) == SPFF_EINVAL and "2..32" in _last_error()
    assert call(n=0) == SPFF_EINVAL and call(n=65) == SPFF_EINVAL
    assert call(tiles=None) == SPFF_EINVAL and call(acc=None) == SPFF_EINVAL
    assert call(tab=None) == SPFF_EINVAL
    for i in range(3):
        w = [p, p, p]
        w[i] = None
        assert call(w=tuple(w)) == SPFF_EINVAL
    assert call(tab=_tab((0, 0, 0, 8))) == SPFF_EINVAL
    assert call(roi=(2, 2, 5)) == SPFF_ESHAPE
    assert call(tab=_tab((0, 3, 0, 0))) == SPFF_ESHAPE
    assert call(tab=_tab((0, 0, 0, 0), (-1, 0, 0, 0)), n=2) == SPFF_ESHAPE


def test_tile_finalize_refusals():
    L = E.lib()
    p, q = _refusal_args()

    def call(acc=p, K=4, n=(p, p, p), flips=1.0, mask=p, scores=None, labels=None, conf=None):
        return L.spff_tile_finalize(acc, 2, 2, 2, K, *n, flips, mask, scores, labels, 0, 0, conf,
                                    None)
    assert call(K=1) == SPFF_EINVAL and call(K=33) == SPFF_EINVAL and "2..32" in _last_error()
    assert call(acc=None) == SPFF_EINVAL and call(mask=None) == SPFF_EINVAL
    assert call(labels=q) == SPFF_EINVAL and call(conf=q) == SPFF_EINVAL  # NULL iff labels NULL
    assert call(scores=p, n=(p, None, p)) == SPFF_EINVAL  # the norms are needed for scores


def _oracle_pair(name, blend, blend_of):
    vol, roi, overlap, _K, _st, _n, _cover = TO.CASES[name]
    tiles, _labels = TO.case_tiles(name)
    tab = TO.table(vol, roi, overlap)
    nvec = TO.norms(vol, roi, overlap, blend)
    return [TO.scores(TO.blend(tiles, tab, vol, blend, blend_of, dt), nvec, 1)
            for dt in (torch.float64, torch.float32)], tiles


@pytest.mark.parametrize("blend_of", ["logits", "probs"])
@pytest.mark.parametrize("blend", T.BLENDS)
@pytest.mark.parametrize("name", list(TO.CASES))
def test_oracle_fp32_mode_against_fp64(name, blend, blend_of):
    (s64, s32), tiles = _oracle_pair(name, blend, blend_of)
    K, cover = TO.CASES[name][3], TO.CASES[name][6]
    assert s32.dtype == torch.float32 and s64.dtype == torch.float64
    assert bool(torch.isfinite(s64).all())
    err = float((s32.double() - s64).abs().max())
    top = float(tiles.abs().max()) if blend_of == "logits" else 1.0
    bound = TO.sum_bound(cover, top, K if blend_of == "probs" else 0)
    print(f"{name} {blend} {blend_of}: fp32 - fp64 {err:.3e} (bound {bound:.3e}, max|ref| "
          f"{float(s64.abs().max()):.3f})")
    assert err <= bound
    # a normalised blend of one constant is that constant: the weights sum to the normaliser
    assert float(s64.abs().max()) <= top * (1 + 1e-6)
    if blend_of == "probs":
        assert float((s64.sum(-1) - 1).abs().max()) <= 1e-6
