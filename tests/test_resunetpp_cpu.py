"""ResUNet++ variant: the CPU oracle (tests/_rupp_oracle.py) pinned to the fixtures the
reference itself produced (tests/golden/make_golden_rupp.py, rupp_*.npz), and the engine
mirror's module tree, flat layout, registry entry and argument checks.  CPU-only."""
import math

import numpy as np
import pytest
import torch

import _rupp_oracle as R
from _compare import check_fixture_grads
from _golden import GOLDEN, load, synth_state_of

NET_FIXTURES = ["rupp_registry_k13", "rupp_core_b8", "rupp_aspp_wide", "rupp_pad_hw"]
LOSS_CASES = ["a", "b", "c", "d", "e"]


def cfg_of(meta):
    return R.RUPPCfg(num_classes=meta["K"], base=meta["base"], in_ch=meta["in_ch"],
                     pad_multiple=meta["pad_multiple"])


def build_lit(meta):
    import innovative3D.models as M
    return M.LitResUNetPP3D_Published(num_classes=meta["K"], in_channels=meta["in_ch"],
                                      base_features=meta["base"],
                                      pad_multiple=meta["pad_multiple"],
                                      ignore_index=meta["ignore_index"])


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_rupp_oracle_matches_reference(name):
    d = load(name)
    meta = d["meta"]
    torch.set_num_threads(8)
    P = R.params_from_state(synth_state_of(d))
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    logits, loss, dice, ce = R.fwd_bwd(P, x, y, cfg_of(meta), meta["ignore_index"])
    ref = d["logits"]
    assert logits.shape == ref.shape
    err = float(np.abs(logits.numpy() - ref).max())
    print(f"{name}: max|dlogit| = {err:.3e} (reference fp32 vs fp64: {float(d['ref_err32']):.3e})")
    assert err <= 2e-5, err
    assert torch.equal(logits.argmax(1), torch.from_numpy(ref).argmax(1))
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
    assert math.isclose(float(ce), float(d["ce"]), rel_tol=1e-5)
    if any(k.startswith(("grad/", "gradhead/")) for k in d):  # rupp_pad_hw: logits, loss and dice only
        check_fixture_grads(d, lambda k: P[k].grad)


def test_rupp_aspp_wide_reaches_every_dilation():
    """The fixture's bottleneck (1 x 1 x 10) has off-centre taps inside for dilation 8."""
    d = load("rupp_aspp_wide")
    k = "backbone.b_aspp.branches.3.weight"
    P = R.params_from_state(synth_state_of(d))
    R.fwd_bwd(P, torch.from_numpy(d["x"]), torch.from_numpy(d["labels"]), cfg_of(d["meta"]), 255)
    g = P[k].grad.numpy().reshape(P[k].shape[0], P[k].shape[1], 27)
    assert np.abs(g[:, :, 12]).max() > 0 and np.abs(g[:, :, 14]).max() > 0
    assert not g[:, :, :9].any() and not g[:, :, 18:].any()  # depth taps read padding only


@pytest.mark.parametrize("case", LOSS_CASES)
def test_rupp_oracle_loss_cases(case):
    z = np.load(GOLDEN / "rupp_loss_small.npz")
    ign = int(z[f"{case}/ignore"])
    ign = None if ign < 0 else ign
    kw = dict(include_bg=bool(int(z[f"{case}/include_bg"])), ce_weight=float(z[f"{case}/ce_weight"]),
              dice_weight=float(z[f"{case}/dice_weight"]))
    lg = torch.from_numpy(z[f"{case}/logits"]).double().requires_grad_(True)
    loss, dice, ce = R.dice_ce_loss(lg, torch.from_numpy(z[f"{case}/labels"]), ign, **kw)
    loss.backward()
    assert math.isclose(float(loss.detach()), float(z[f"{case}/loss"]), rel_tol=1e-12)
    assert math.isclose(float(dice), float(z[f"{case}/dice"]), rel_tol=1e-12)
    assert math.isclose(float(ce), float(z[f"{case}/ce"]), rel_tol=1e-12)
    np.testing.assert_allclose(lg.grad.numpy(), z[f"{case}/dlogits"], rtol=1e-9, atol=1e-15)
    l32, d32, c32 = R.dice_ce_loss(torch.from_numpy(z[f"{case}/logits"]),
                                   torch.from_numpy(z[f"{case}/labels"]), ign, **kw)
    assert math.isclose(float(l32), float(z[f"{case}/loss32"]), rel_tol=1e-5)
    assert math.isclose(float(d32), float(z[f"{case}/dice32"]), rel_tol=1e-5)
    assert math.isclose(float(c32), float(z[f"{case}/ce32"]), rel_tol=1e-5)


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_rupp_layouts_match_reference_state_dict(name):
    """Module mirror, oracle and engine plan all use the reference's names, shapes, order."""
    from innovative3D import _engine as E
    d = load(name)
    meta = d["meta"]
    ref = d["state_shapes"]
    m = build_lit(meta)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys()) == [str(k) for k in d["state_keys"]]
    assert all(tuple(sd[k].shape) == tuple(ref[k]) for k in sd)
    named = [(k, tuple(v.shape)) for k, v in m.named_parameters()]
    assert [k for k, _s in named] == [str(k) for k in d["param_names"]]
    assert list(R.param_shapes(cfg_of(meta)).items()) == named
    assert "backbone.b_aspp_out.skip.weight" not in sd
    plan = E.RUPPPlan(batch=1, in_ch=meta["in_ch"], depth=16, height=32, width=32,
                      num_classes=meta["K"], base=meta["base"])
    assert [(n, s) for n, s, _o, _k in plan.params] == named
    assert len(plan.params) == 118
    offs = [o for _n, _s, o, _k in plan.params]
    assert all(a < b for a, b in zip(offs, offs[1:]))
    assert plan.nfloats == sum(int(np.prod(s)) for _n, s in named)
    assert plan.nfloats == offs[-1] + plan.params[-1][3] and plan.ws_bytes > 0


def test_rupp_registry_entry(monkeypatch):
    from innovative3D import config as C
    import innovative3D.models as M
    i = C.VARIANT_NAMES.index("ResUNet++")
    assert C.VARIANT_NAMES[i - 1] == "3DUNet" and C.VARIANT_NAMES[i + 1] == "SwinUNETR"
    name, factory, dm, ck = C.variant("ResUNet++")
    lit = factory()
    assert isinstance(lit, M.LitResUNetPP3D_Published) and callable(dm)
    want = load("rupp_registry_k13")["meta"]["hparams"]
    assert {k: lit.hparams[k] for k in want} == want and set(lit.hparams) == set(want)
    assert lit.backbone.out_ch == 16 and lit.head.out_channels == 13
    opt = lit.configure_optimizers()
    assert type(opt) is torch.optim.Adam
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"]) == (1e-4, 1e-5)
    assert ck.name == "ResUNet++"
    monkeypatch.setenv("INNOVATIVE3D_VARIANT", "ResUNet++")
    assert [v[0] for v in C.selected_variants()] == ["ResUNet++"]


def test_rupp_plan_rejects_bad_arguments():
    from innovative3D import _engine as E
    ok = dict(batch=1, in_ch=1, depth=16, height=32, width=32, num_classes=13, base=16)
    E.RUPPPlan(**ok)
    for dim in ("depth", "height", "width"):
        with pytest.raises(E.SpffError, match="multiples of 16"):
            E.RUPPPlan(**{**ok, dim: 24})
    with pytest.raises(E.SpffError, match="base must be a multiple of 8"):
        E.RUPPPlan(**{**ok, "base": 12})
    for bad in ({"in_ch": 0}, {"in_ch": 9}):
        with pytest.raises(E.SpffError, match="in_ch"):
            E.RUPPPlan(**{**ok, **bad})
    for bad in ({"num_classes": 1}, {"num_classes": 33}):
        with pytest.raises(E.SpffError, match="num_classes"):
            E.RUPPPlan(**{**ok, **bad})
    with pytest.raises(E.SpffError, match="one voxel per sample"):
        E.RUPPPlan(**{**ok, "depth": 16, "height": 16, "width": 16})
    E.RUPPPlan(**{**ok, "num_classes": 32, "base": 24, "in_ch": 8})
    E.RUPPPlan(**{**ok, "num_classes": 2, "height": 16, "width": 16, "depth": 32})


def test_rupp_runs_only_on_device():
    import innovative3D.models as M
    from innovative3D import _engine as E
    m = M.LitResUNetPP3D_Published(num_classes=3, base_features=8)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 16, 16, 32))
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        m._loss(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 2, 4, 4).long())
    with pytest.raises(NotImplementedError, match="parameters only"):
        m.backbone(torch.zeros(1, 1, 16, 16, 32))


def test_rupp_unbuilt_cases_are_refused():
    import innovative3D.models as M
    with pytest.raises(NotImplementedError, match="num_classes == 1"):
        M.LitResUNetPP3D_Published(num_classes=1)
    for pm in (8, 24):
        with pytest.raises(NotImplementedError, match="multiple of 16"):
            M.LitResUNetPP3D_Published(num_classes=3, pad_multiple=pm)
    M.LitResUNetPP3D_Published(num_classes=3, base_features=8, pad_multiple=32)


def test_rupp_constructor_defaults_are_the_reference_ones():
    import inspect
    import innovative3D.models as M
    sig = inspect.signature(M.LitResUNetPP3D_Published.__init__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == [("num_classes", inspect.Parameter.empty), ("in_channels", 1),
                   ("base_features", 16), ("include_bg_in_dice", False), ("ignore_index", None),
                   ("ce_weight", 0.5), ("dice_weight", 0.5), ("lr", 1e-3), ("weight_decay", 1e-5),
                   ("pad_multiple", 16)]


def test_unified_loss_patches_rupp(capsys):
    import innovative3D.models as M
    from innovative3D.unified_loss import apply_unified_loss
    steps = ("training_step", "validation_step", "test_step")
    lits = [c for c in vars(M).values()
            if isinstance(c, type) and issubclass(c, M.pl.LightningModule)]
    saved = {c: {k: vars(c)[k] for k in steps if k in vars(c)} for c in lits}
    try:
        patched = apply_unified_loss()
        assert "LitResUNetPP3D_Published" in patched
        assert M.LitResUNetPP3D_Published.training_step.__module__ == "innovative3D.unified_loss"
        assert M.LitResUNetPP3D_Published.test_step.__module__ == "innovative3D.unified_loss"
    finally:  # the classes as they were: own steps restored, added ones removed
        for c, own in saved.items():
            for k in steps:
                if k in own:
                    setattr(c, k, own[k])
                elif k in vars(c):
                    delattr(c, k)
