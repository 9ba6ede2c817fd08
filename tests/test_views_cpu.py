"""Prediction views and overlay figures (csrc/views.hip, helpers.prediction_views /
render_overlays / write_png), the part that needs no GPU: the ABI is declared and exported,
every refusal comes before a device call, there is no CPU fallback, the PNG writer round-trips
and replaces atomically, a numpy restatement of the definitions reproduces the fixtures, and
the generated palette is usable."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

import _views_oracle as VO
from innovative3D import _engine as E
from innovative3D import helpers as Hh

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAMES = ("spff_pred_views_ws_bytes", "spff_pred_views", "spff_input_views", "spff_overlay_rgb")
EINVAL = -1


def test_header_declares_and_library_exports():
    src = (ROOT / "include" / "spff.h").read_text()
    L = E.lib()
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert hasattr(L, n) and n in E.EXPORTED, n
    for n in ("prediction_views", "render_overlays", "write_png"):
        assert n in Hh.__all__ and callable(getattr(Hh, n))


def _refused(rc):
    """SPFF_EINVAL with a message (where there is no device, a call that got as far as a
    launch would come back as SPFF_EHIP instead)."""
    msg = E.lib().spff_last_error()
    return rc == EINVAL and bool(msg) and len(msg.decode()) > 10


def test_pred_views_refusals_come_before_any_device_call():
    L = E.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused
    ok = dict(B=1, D=4, H=8, W=8, K=5, split=0)

    def call(ptrs=(p,) * 6, **kw):
        a = {**ok, **kw}
        lg, cp, al, mp, mi, ws = ptrs
        return L.spff_pred_views(lg, a["B"], a["D"], a["H"], a["W"], a["K"], a["split"], cp, al,
                                 mp, mi, ws, None)

    for i in range(6):
        assert _refused(call(tuple(None if j == i else p for j in range(6)))), i
    for bad in (dict(K=0), dict(K=33), dict(K=-1), dict(B=0), dict(D=0), dict(H=0), dict(W=0),
                dict(W=-3), dict(split=-1), dict(split=5)):
        assert _refused(call(**bad)), bad
        if "split" not in bad:
            a = {**ok, **bad}
            assert L.spff_pred_views_ws_bytes(a["B"], a["D"], a["H"], a["W"], a["K"]) == 0
    assert "depth_split" in L.spff_last_error().decode()
    assert L.spff_pred_views_ws_bytes(1, 4, 8, 8, 5) > 0


def test_input_views_and_overlay_refusals_come_before_any_device_call():
    L = E.lib()
    p = ctypes.c_void_p(4096)
    for i in range(4):
        ptrs = [None if j == i else p for j in range(4)]
        assert _refused(L.spff_input_views(ptrs[0], 1, 1, 4, 8, 8, ptrs[1], ptrs[2], ptrs[3], None)), i
    for dims in ((0, 1, 4, 8, 8), (1, 0, 4, 8, 8), (1, 1, 0, 8, 8), (1, 1, 4, 0, 8), (1, 1, 4, 8, 0)):
        assert _refused(L.spff_input_views(p, *dims, p, p, p, None)), dims
    # labels_center (argument 3) may be NULL; every other pointer may not
    for i in (0, 1, 2, 4, 5, 6, 7, 8):
        a = [None if j == i else p for j in range(9)]
        assert _refused(L.spff_overlay_rgb(*a[:8], 1, 8, 8, 5, a[8], None)), i
    for B, H, W, K in ((0, 8, 8, 5), (1, 0, 8, 5), (1, 8, 0, 5), (1, 8, 8, 0), (1, 8, 8, 33)):
        assert _refused(L.spff_overlay_rgb(p, p, p, None, p, p, p, p, B, H, W, K, p, None)), (B, H, W, K)


def test_no_cpu_fallback():
    lg = torch.zeros(1, 3, 2, 4, 4)
    x = torch.zeros(1, 1, 2, 4, 4)
    img, u8 = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        E.pred_views(lg.permute(0, 2, 3, 4, 1))
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        E.input_views(x)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        E.overlay_rgb(img, img, torch.zeros(1, 4), None, u8, u8, img,
                      torch.zeros(256, 3, dtype=torch.uint8), 3)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        Hh.prediction_views(lg)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        Hh.render_overlays(x, None, lg)


def test_write_png_round_trips_and_replaces_atomically(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(7, 45, 3), dtype=np.uint8)
    b = rng.integers(0, 256, size=(3, 5, 3), dtype=np.uint8)
    path = tmp_path / "sub" / "strip.png"
    assert Hh.write_png(path, a) == path
    assert np.array_equal(VO.decode_png(path), a)
    Hh.write_png(path, torch.from_numpy(b))       # an existing file is replaced ...
    assert np.array_equal(VO.decode_png(path), b)
    assert [q.name for q in path.parent.iterdir()] == ["strip.png"]  # ... and no temporary stays
    for bad in (a.astype(np.float32), a[..., 0], a[..., :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            Hh.write_png(tmp_path / "bad.png", bad)
    assert not (tmp_path / "bad.png").exists()


def test_write_png_moves_a_finished_file_into_place(tmp_path, monkeypatch):
    import os
    seen = []
    real = os.replace

    def spy(src, dst):
        seen.append((pathlib.Path(src).name, pathlib.Path(dst).name,
                     VO.decode_png(src).shape))  # complete before it takes the final name
        return real(src, dst)
    monkeypatch.setattr(os, "replace", spy)
    Hh.write_png(tmp_path / "o.png", np.zeros((2, 3, 3), np.uint8))
    assert seen == [("o.png.part.png", "o.png", (2, 3, 3))]


@pytest.mark.parametrize("name", VO.FIXTURES)
def test_numpy_restatement_reproduces_the_fixture(name):
    d = VO.load(name)
    m = d["meta"]
    lg = d["logits"]
    assert lg.shape == (m["B"], m["K"], m["D"], m["H"], m["W"]) and lg.dtype == np.float32
    assert np.array_equal(d["summary_pred"], d["mip_pred"])  # the same array in the reference
    centre_ok, mip_ok, block = VO.comparable(d)
    # the stored near-tie shares are what the fp64 values give, and small enough
    assert float(d["center_tie_share"]) == pytest.approx((~centre_ok).mean(), abs=1e-12)
    assert float(d["mip_tie_share"]) == pytest.approx((~mip_ok).mean(), abs=1e-12)
    assert float(d["center_tie_share"]) <= VO.MAX_TIES and float(d["mip_tie_share"]) <= VO.MAX_TIES
    tol_a, tol_m = VO.prob_tol(d)
    for dtype, sfx in ((np.float32, ""), (np.float64, "64")):
        cp, al, mip, mp = VO.views(lg.astype(dtype))
        assert al.dtype == dtype and mip.dtype == dtype
        assert np.array_equal(cp[centre_ok], d["center_pred" + sfx][centre_ok])
        assert np.array_equal(mp[mip_ok], d["mip_pred" + sfx][mip_ok])
        assert np.abs(al - d["alpha_center64"]).max() <= (tol_a if dtype == np.float32 else 1e-12)
        assert np.abs(mip - d["mip_prob64"]).max() <= (tol_m if dtype == np.float32 else 1e-12)
    # the block: exact 1.0s in fp32, the lowest class present along depth wins
    bw = int(d["block_w"])
    assert bw == m["W"] // 3 and bw >= 1
    cp, al, mip, mp = VO.views(lg)
    assert np.all(mip[..., :bw].max(axis=1) == np.float32(1.0)) and np.all(al[..., :bw] == 1.0)
    lowest = lg[..., :bw].argmax(axis=1).min(axis=1)
    assert np.array_equal(mp[..., :bw], lowest) and np.array_equal(d["mip_pred"][..., :bw], lowest)
    if m["D"] > 1:
        assert ((mip[..., :bw] == 1.0).sum(axis=1) > 1).any()  # several exact 1.0s to choose from
    # the reference's own rounding error is of the size the tolerance rule expects
    assert 0 < float(d["e32_alpha"]) < 2e-6 and 0 < float(d["e32_mip"]) < 2e-6


def test_fixtures_are_the_shapes_they_are_for():
    L = E.lib()
    shapes = {n: tuple(VO.load(n)["meta"][k] for k in "BKDHW") for n in VO.FIXTURES}
    assert shapes == {"views_k13_d5": (2, 13, 5, 24, 20), "views_ragged": (1, 4, 7, 9, 33),
                      "views_k32_d3": (1, 32, 3, 8, 8), "views_deep": (1, 13, 64, 16, 16),
                      "views_d1": (1, 3, 1, 8, 16)}
    # the automatic split of views_deep is above 1: its workspace holds more than one slab
    B, K, D, H, W = shapes["views_deep"]
    assert L.spff_pred_views_ws_bytes(B, D, H, W, K) >= 2 * B * H * W * K * 4
    # the workspace stays a fraction of the logits at the sizes that matter
    for B, K, D, H, W in ((2, 13, 128, 128, 128), (2, 13, 5, 512, 512), (1, 13, 512, 512, 512)):
        assert L.spff_pred_views_ws_bytes(B, D, H, W, K) <= B * K * D * H * W * 4 // 4 + B * K * H * W * 4 + 64


def test_palette():
    for K in (1, 2, 13, 32):
        pal = Hh.default_palette(K)
        assert sorted(pal) == list(range(K)) and pal[0] == (0, 0, 0)
        assert len(set(pal.values())) == K
        assert all(0 <= v <= 255 for col in pal.values() for v in col)
        tab = Hh.color_table(None, K)
        assert tab.dtype == torch.uint8 and tuple(tab.shape) == (256, 3)
        assert not tab[K:].any() and [tuple(r) for r in tab[:K].tolist()] == [pal[c] for c in range(K)]
    own = Hh.color_table({1: (255, 0, 0), 7: (1, 2, 3)}, 13)  # the shape config.label_colors has
    assert own[1].tolist() == [255, 0, 0] and own[7].tolist() == [1, 2, 3]
    assert not own[0].any() and not own[2].any()  # a class without an entry is black
    with pytest.raises(ValueError):
        Hh.color_table({1: (256, 0, 0)}, 3)


def test_viz_settings_default_off(monkeypatch):
    """VIZ_EVERY_N_EPOCHS defaults to 0 (existing runs write what they wrote); FAST_SKIP_VIZ=1
    turns the figures off whatever it says (train.py:22, 1138)."""
    import sys
    monkeypatch.syspath_prepend(str(ROOT / "spff-unet-spcct_amd"))
    sys.modules.pop("train", None)
    import train as T
    for k in ("VIZ_EVERY_N_EPOCHS", "VIZ_MAX_ITEMS", "FAST_SKIP_VIZ"):
        monkeypatch.delenv(k, raising=False)
    S = T.Settings()
    assert S.viz_every == 0 and S.viz_max_items == 2
    monkeypatch.setenv("VIZ_EVERY_N_EPOCHS", "3")
    assert T.Settings().viz_every == 3
    monkeypatch.setenv("FAST_SKIP_VIZ", "1")
    assert T.Settings().viz_every == 0
    sys.modules.pop("train", None)
