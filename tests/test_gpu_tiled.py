"""Sliding-window inference on the device (csrc/tile.hip, helpers.predict_tiled): the three
kernels against torch slicing and the fp64 oracle of tests/_tile_oracle.py on the cases of
DESIGN §8.3, the order, batching, flip and replay guarantees, and predict_tiled end to end
against the same kernels driven by hand.  Marked gpu."""
import numpy as np
import pytest
import torch

import _compare as CMP
import _spff_checks as SC
import _tile_oracle as TO
from innovative3D import _engine as E
from innovative3D import helpers as Hh
from innovative3D import tiling as T

pytestmark = pytest.mark.gpu
_CACHE = {}
BLENDS = ("gaussian", "constant")
KINDS = ("logits", "probs")


def _case(name):
    """the case's table, tiles and labels, made once and left unchanged"""
    if name not in _CACHE:
        vol, roi, overlap, K, _st, n, _cover = TO.CASES[name]
        tiles, labels = TO.case_tiles(name)
        tab = T.window_table(vol, roi, overlap)
        assert len(tab) == n
        _CACHE[name] = {"vol": vol, "r": T.clamp_roi(vol, roi), "overlap": overlap, "K": K,
                        "tab": tab, "tiles": tiles, "tiles_dev": tiles.cuda(), "labels": labels}
    return _CACHE[name]


def _oracle(name, blend, blend_of):
    """(fp64 scores, fp32 scores) of the CPU oracle, once per combination"""
    key = (name, blend, blend_of)
    if key not in _CACHE:
        c = _case(name)
        vol, roi, overlap = TO.CASES[name][:3]
        tab = TO.table(vol, roi, overlap)
        nvec = TO.norms(vol, roi, overlap, blend)
        _CACHE[key] = tuple(TO.scores(TO.blend(c["tiles"], tab, vol, blend, blend_of, dt), nvec, 1)
                            for dt in (torch.float64, torch.float32))
    return _CACHE[key]


def _weights(r, blend):
    return tuple(torch.from_numpy(T.axis_weights(ri, blend)).cuda() for ri in r)


def _accumulate(c, blend, blend_of, per_call, tiles=None, tab=None):
    tiles = c["tiles_dev"] if tiles is None else tiles
    tab = c["tab"] if tab is None else tab
    acc = torch.zeros(tuple(c["vol"]) + (c["K"],), device="cuda")
    w = _weights(c["r"], blend)
    for i0, i1 in T.batches(len(tab), per_call):
        E.tile_accumulate(tiles[i0:i1], tab[i0:i1], w, acc, softmax=blend_of == "probs")
    return acc


@pytest.mark.parametrize("bits", [0, 1, 6, 7])
@pytest.mark.parametrize("name", list(TO.CASES))
def test_gather_is_slicing_plus_flip(name, bits):
    c = _case(name)
    C = 3
    g = torch.Generator().manual_seed(17)
    x = torch.randn(C, *c["vol"], generator=g)
    tab = c["tab"].copy()
    tab[:, 3] = bits
    rd, rh, rw = c["r"]
    xd = x.cuda()
    got = torch.cat([E.tile_gather(xd, tab[i0:i1], c["r"])
                     for i0, i1 in T.batches(len(tab), T.MAX_WINDOWS)]).cpu()
    want = torch.stack([torch.flip(x[:, z:z + rd, y:y + rh, xx:xx + rw], TO.flip_dims(bits, 1))
                        for z, y, xx, _f in tab.tolist()])
    assert got.shape == want.shape and torch.equal(got, want)


def test_gather_fills_only_the_first_n_slots():
    c = _case("overlap_3d")
    x = torch.randn(2, *c["vol"], generator=torch.Generator().manual_seed(3)).cuda()
    out = torch.full((5, 2) + c["r"], -7.0, device="cuda")
    E.tile_gather(x, c["tab"][:5], c["r"], out=out, n=3)
    assert torch.equal(out[:3], E.tile_gather(x, c["tab"][:3], c["r"]))
    assert bool((out[3:] == -7.0).all())


@pytest.mark.parametrize("blend_of", KINDS)
@pytest.mark.parametrize("blend", BLENDS)
@pytest.mark.parametrize("name", list(TO.CASES))
def test_blend_against_the_oracle(name, blend, blend_of):
    c = _case(name)
    K, vol = c["K"], c["vol"]
    ref64, ref32 = _oracle(name, blend, blend_of)
    acc = _accumulate(c, blend, blend_of, T.MAX_WINDOWS)
    norms = tuple(torch.from_numpy(v).cuda()
                  for v in T.norm_vectors(vol, c["r"], c["overlap"], blend))
    keep = acc.clone()
    mask, conf, scores = E.tile_finalize(acc, norms, 1, c["labels"], 255, scores=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)  # scores went to their own tensor
    assert mask.dtype == torch.uint8 and mask.shape == tuple(vol)
    assert scores.shape == acc.shape and conf.shape == (K, K + 1) and conf.dtype == torch.int64
    assert bool(torch.isfinite(scores).all())
    bound, e32, ref_max = CMP.fp32_bound(ref64, ref32)
    err = float((scores.cpu().double() - ref64).abs().max())
    print(f"{name} {blend} {blend_of}: |scores - fp64| {err:.3e} (bound {bound:.3e}, torch fp32 "
          f"{e32:.3e}, max|ref| {ref_max:.3f})")
    assert err <= bound
    # class map: flips against the oracle only at its near-ties, and those are rare
    ref_kf = ref64.permute(3, 0, 1, 2)[None].numpy()
    near = CMP.near_tie_mask(ref_kf, 2 * bound)[0]
    flips = mask.cpu().numpy() != ref_kf[0].argmax(0)
    print(f"{name} {blend} {blend_of}: near ties {near.mean():.3%}, flips {int(flips.sum())}")
    assert near.mean() <= 1e-3
    assert not (flips & ~near).any()
    # exact: the first maximum of the accumulator and the confusion counts of the same rows
    assert torch.equal(mask.cpu().long(), torch.argmax(acc.cpu(), -1))
    assert torch.equal(conf, E.confusion(acc, c["labels"], K, 255))
    assert int(conf[:, K].sum()) > 0  # labels outside [0, K) land in column K
    _m, conf_all, none = E.tile_finalize(acc, labels=c["labels"], ignore_index=None)
    assert none is None and torch.equal(_m, mask)
    assert torch.equal(conf_all, E.confusion(acc, c["labels"], K, None))
    assert int(conf_all.sum()) == mask.numel() > int(conf.sum())
    # in place: the scores may overwrite the accumulator
    m2, c2, s2 = E.tile_finalize(acc, norms, 1, scores=acc)
    assert c2 is None and s2 is acc and torch.equal(m2, mask) and torch.equal(acc, scores)


@pytest.mark.parametrize("blend_of", KINDS)
@pytest.mark.parametrize("name", list(TO.CASES))
def test_order_and_batching_do_not_change_a_bit(name, blend_of):
    c = _case(name)
    base = _accumulate(c, "gaussian", blend_of, 64)
    for per_call in (1, 5, 64):
        assert torch.equal(_accumulate(c, "gaussian", blend_of, per_call), base), per_call


@pytest.mark.parametrize("bits", [1, 2, 4, 7])
@pytest.mark.parametrize("name", list(TO.CASES))
def test_flipped_windows_accumulate_mirrored_back(name, bits):
    c = _case(name)
    tab = c["tab"].copy()
    tab[:, 3] = bits
    mirrored = torch.flip(c["tiles_dev"], TO.flip_dims(bits, 1)).contiguous()
    for blend_of in KINDS:
        got = _accumulate(c, "gaussian", blend_of, 64, tab=tab)
        want = _accumulate(c, "gaussian", blend_of, 64, tiles=mirrored)
        assert torch.equal(got, want)
        assert not torch.equal(got, _accumulate(c, "gaussian", blend_of, 64))


def test_more_tiles_than_windows_are_left_out():
    c = _case("overlap_3d")
    w = _weights(c["r"], "gaussian")
    acc = torch.zeros(tuple(c["vol"]) + (c["K"],), device="cuda")
    E.tile_accumulate(c["tiles_dev"], c["tab"], w, acc, n=7)
    assert torch.equal(acc, _accumulate(c, "gaussian", "logits", 64, tiles=c["tiles_dev"][:7],
                                        tab=c["tab"][:7]))


def test_engine_wrappers_refuse_before_the_device():
    c = _case("overlap_3d")
    w = _weights(c["r"], "gaussian")
    acc = torch.zeros(tuple(c["vol"]) + (c["K"],), device="cuda")
    bad = c["tab"].copy()
    bad[3, 2] = c["vol"][2] - c["r"][2] + 1  # one voxel over the edge
    with pytest.raises(E.SpffError, match="inside"):
        E.tile_accumulate(c["tiles_dev"], bad, w, acc)
    with pytest.raises(E.SpffError, match="inside"):
        E.tile_gather(torch.zeros((1,) + tuple(c["vol"]), device="cuda"), bad, c["r"])
    bad = c["tab"].copy()
    bad[0, 3] = 8
    with pytest.raises(E.SpffError, match="flip"):
        E.tile_accumulate(c["tiles_dev"], bad, w, acc)
    assert not bool(acc.any())
    with pytest.raises(E.SpffError):
        E.tile_accumulate(c["tiles_dev"].cpu(), c["tab"], w, acc)


def test_graph_replay_equals_eager():
    c = _case("overlap_3d")
    K, vol = c["K"], c["vol"]
    w = _weights(c["r"], "gaussian")
    norms = tuple(torch.from_numpy(v).cuda()
                  for v in T.norm_vectors(vol, c["r"], c["overlap"], "gaussian"))
    labels = c["labels"].cuda()
    t1 = c["tiles_dev"]
    t2 = torch.roll(t1, shifts=(1, 2), dims=(0, 4)).contiguous()

    def run(tiles, acc, mask, conf, scores):
        acc.zero_()
        E.tile_accumulate(tiles, c["tab"], w, acc, softmax=True)
        return E.tile_finalize(acc, norms, 1, labels, 255, scores=scores, mask=mask, conf=conf)

    def fresh():
        return (torch.empty(tuple(vol) + (K,), device="cuda"),
                torch.empty(tuple(vol), dtype=torch.uint8, device="cuda"),
                torch.empty(K * (K + 1), dtype=torch.int64, device="cuda"),
                torch.empty(tuple(vol) + (K,), device="cuda"))
    ref1 = [t.clone() for t in run(t1, *fresh())]
    ref2 = [t.clone() for t in run(t2, *fresh())]
    assert not torch.equal(ref1[0], ref2[0])
    buf = t1.clone()
    bufs = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(buf, *bufs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # single stream: no allocation or sync inside the calls
        out = run(buf, *bufs)
    for src, ref in ((t1, ref1), (t2, ref2), (t1, ref1)):
        buf.copy_(src)  # overwritten in place
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ end to end --
def _by_hand(forward, x, roi, overlap, wb, mirror, blend, labels, ign):
    """predict_tiled's result from ``forward(x_windows)`` -> [wb, K, rd, rh, rw] and the
    engine's tile entries, with predict_tiled's batching"""
    B, _C, D, H, W = x.shape
    r = T.clamp_roi((D, H, W), roi)
    tab = T.window_table((D, H, W), r, overlap, mirror)
    w = _weights(r, blend)
    norms = tuple(torch.from_numpy(v).cuda() for v in T.norm_vectors((D, H, W), r, overlap, blend))
    masks, scores, conf = [], [], None
    for b in range(B):
        acc = None
        for i0, i1 in T.batches(len(tab), wb):
            rows = np.concatenate([tab[i0:i1], np.repeat(tab[i1 - 1:i1], wb - (i1 - i0), axis=0)])
            with torch.no_grad():
                lg = forward(E.tile_gather(x[b].contiguous(), rows, r))
            tiles = lg.permute(0, 2, 3, 4, 1).contiguous()
            if acc is None:
                acc = torch.zeros((D, H, W, tiles.shape[-1]), device="cuda")
            E.tile_accumulate(tiles, tab[i0:i1], w, acc)
        m, cf, s = E.tile_finalize(acc, norms, len(T.flip_passes(mirror)), labels[b], ign,
                                   scores=True)
        masks.append(m)
        scores.append(s.permute(3, 0, 1, 2))
        conf = cf if conf is None else conf + cf
    return torch.stack(masks), conf, torch.stack(scores)


def _labels(shape, K, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, K, shape, generator=g)
    y[torch.rand(shape, generator=g) < 0.05] = 255
    return y.cuda()


def _assert_same(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


CORE_CASES = {
    "base8": dict(shape=(1, 5, 12, 24, 32), base=8, K=6, roi=(8, 16, 16), overlap=0.5),
    "stream32": dict(shape=(2, 1, 5, 24, 40), base=32, K=13, roi=(5, 16, 16), overlap=0.25),
}


def _core(case, depth):
    c = CORE_CASES[case]
    core, _st = SC.synth_core(c["K"], c["base"], c["shape"][1], depth, seed=11, mask_jitter=0.25)
    x = torch.randn(*c["shape"], generator=torch.Generator().manual_seed(5)).cuda()
    return core.cuda().eval(), x, _labels((c["shape"][0],) + c["shape"][2:], c["K"], 9)


@pytest.mark.parametrize("case,wb,mirror", [("base8", 1, ()), ("base8", 2, ()), ("base8", 5, ()),
                                            ("base8", 2, (2,)), ("stream32", 1, ()),
                                            ("stream32", 4, ())])
def test_predict_tiled_on_the_core(case, wb, mirror):
    c = CORE_CASES[case]
    core, x, y = _core(case, c["roi"][0])
    got = core.predict_tiled(x, c["roi"], overlap=c["overlap"], window_batch=wb,
                             mirror_axes=mirror, labels=y, ignore_index=255, return_scores=True)
    torch.cuda.synchronize()
    plan = core._infer_plan
    assert plan.layout == "infer" and plan.cfg.batch == wb
    assert tuple((plan.cfg.depth, plan.cfg.height, plan.cfg.width)) == tuple(c["roi"])
    plans = [p for lru in E._OWNER_PLANS[core].values() for p in lru.values()]
    assert plans == [plan]  # the partial last batch ran on the same plan
    mask, conf, scores = got
    B, _C, D, H, W = c["shape"]
    assert mask.shape == (B, D, H, W) and mask.dtype == torch.uint8
    assert conf.shape == (c["K"], c["K"] + 1) and scores.shape == (B, c["K"], D, H, W)
    assert int(conf.sum()) == int((y != 255).sum())
    _assert_same(got, _by_hand(core, x, c["roi"], c["overlap"], wb, mirror, "gaussian", y, 255))
    # the mask alone, and again: the same bits
    assert torch.equal(core.predict_tiled(x, c["roi"], overlap=c["overlap"], window_batch=wb,
                                          mirror_axes=mirror), mask)


def test_one_window_of_the_whole_volume_is_predict():
    c = CORE_CASES["base8"]
    core, x, y = _core("base8", c["shape"][2])
    mask, conf, scores = core.predict_tiled(x, (16, 32, 32), blend="constant", labels=y,
                                            ignore_index=255, return_scores=True)
    want_mask, want_conf = core.predict(x, labels=y, ignore_index=255)
    assert torch.equal(mask, want_mask) and torch.equal(conf, want_conf)
    with torch.no_grad():
        assert torch.equal(scores, core(x))


def test_lit_wrappers():
    import innovative3D.models as M
    c = CORE_CASES["base8"]
    lit = M.LitSPCT_EFiLM_FourierGate(num_classes=c["K"], base=8, in_channels=5)
    core, x, y = _core("base8", c["roi"][0])
    lit.model = core
    assert M.supports_predict(lit)
    _assert_same(lit.predict_tiled(x, c["roi"], window_batch=2, labels=y, ignore_index=255),
                 core.predict_tiled(x, c["roi"], window_batch=2, labels=y, ignore_index=255))
    with pytest.raises(NotImplementedError):
        M._LitSPCT_Base.predict_tiled(lit, x, c["roi"])


@pytest.mark.parametrize("fast", ["1", "0"])
def test_evaluate_rows_with_roi(monkeypatch, fast):
    """test.py evaluate with --roi: the rows come from predict_tiled's counts and, for the
    ranking metrics, its blended scores taken as logits"""
    import sys

    import innovative3D.models as M
    from innovative3D.synthetic import SyntheticSPCCT
    monkeypatch.setenv("FAST_SIMPLE_METRICS", fast)
    sys.modules.pop("test", None)
    import test as TT
    K = 6
    torch.manual_seed(5)
    model = M.LitSPCT_EFiLM_FourierGate(num_classes=K, base=8).cuda()
    TT.materialize_lazy(model, 5, "cuda")
    ds = SyntheticSPCCT(n=2, in_ch=1, depth=5, height=24, width=40, num_classes=K, seed=11)
    tiled = {"roi": (5, 16, 16), "overlap": 0.25, "window_batch": 4, "mirror_axes": (2,)}
    rows = TT.evaluate(model, ds, K, torch.device("cuda"), tiled)
    assert model.model._infer_plan.layout == "infer" and model.model._infer_plan.cfg.batch == 4
    assert len(rows) == 2 * K and list(rows[0]) == TT.detail_fields()
    want = []
    for i in range(len(ds)):
        x, y = ds[i]
        x, y = x[None].cuda(), y[None].cuda()
        _mask, conf, scores = model.predict_tiled(x, labels=y, ignore_index=255,
                                                  return_scores=True, **tiled)
        dice, sens, spec, *_ = Hh.metrics_from_confusion(conf.cpu().numpy(), K, int(y.numel()))
        rm = Hh.ranking_metrics(scores, y, K, per_sample=True) if fast == "0" else None
        for c in range(K):
            row = {"volume": i, "class": c, "dice": dice[c], "sens": sens[c], "spec": spec[c]}
            if rm is not None:
                row.update({k: rm[k][0][c] for k in TT.RANK_FIELDS})
            want.append(row)
    assert repr(rows) == repr(want)  # (NaN-safe: absent classes carry nan)


def test_generic_path_on_r2unet():
    import innovative3D.models as M
    torch.manual_seed(21)
    lit = M.LitR2UNet3D_Published(num_classes=5, in_channels=1, base_features=8).cuda().eval()
    assert not M.supports_predict(lit)
    x = torch.randn(1, 1, 16, 32, 48, generator=torch.Generator().manual_seed(6)).cuda()
    y = _labels((1, 16, 32, 48), 5, 4)
    roi = (16, 16, 16)
    assert len(T.window_table(x.shape[2:], roi, 0.0)) == 6
    got = Hh.predict_tiled(lit, x, roi, overlap=0.0, window_batch=4, labels=y, ignore_index=255,
                           return_scores=True)
    _assert_same(got, _by_hand(lit, x, roi, 0.0, 4, (), "gaussian", y, 255))
    probs = Hh.predict_tiled(lit, x, roi, overlap=0.0, blend_of="probs", return_scores=True)[1]
    assert float((probs.sum(1) - 1).abs().max()) <= 1e-5
