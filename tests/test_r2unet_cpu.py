"""R2UNet3D variant: the CPU oracle (tests/_r2u_oracle.py) pinned to the fixtures the
reference itself produced (tests/golden/make_golden_r2u.py, r2u_*.npz), and the engine
mirror's module tree, flat layout, registry entry and argument checks.  CPU-only."""
import math

import numpy as np
import pytest
import torch

import _r2u_oracle as R
from _compare import check_fixture_grads
from _golden import load, synth_state_of

NET_FIXTURES = ["r2u_registry_k13", "r2u_core_b8_t3", "r2u_pad_hw"]
LOSS_CASES = ["a", "b", "c", "d"]


def cfg_of(meta):
    return R.R2UCfg(num_classes=meta["K"], base=meta["base"], in_ch=meta["in_ch"], t=meta["t"],
                    pad_multiple=meta["pad_multiple"])


def build_lit(meta):
    import innovative3D.models as M
    return M.LitR2UNet3D_Published(num_classes=meta["K"], in_channels=meta["in_ch"],
                                   base_features=meta["base"], t=meta["t"],
                                   pad_multiple=meta["pad_multiple"],
                                   ignore_index=meta["ignore_index"])


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_r2u_oracle_matches_reference(name):
    d = load(name)
    meta = d["meta"]
    torch.set_num_threads(8)
    P = R.params_from_state(synth_state_of(d))
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    logits, loss, dice = R.fwd_bwd(P, x, y, cfg_of(meta), meta["ignore_index"])
    ref = d["logits"]
    assert logits.shape == ref.shape
    err = float(np.abs(logits.numpy() - ref).max())
    print(f"{name}: max|dlogit| = {err:.3e} (reference fp32 vs fp64: {float(d['ref_err32']):.3e})")
    assert err <= 2e-5, err
    assert torch.equal(logits.argmax(1), torch.from_numpy(ref).argmax(1))
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
    if any(k.startswith(("grad/", "gradhead/")) for k in d):  # r2u_pad_hw: logits, loss and dice only
        check_fixture_grads(d, lambda k: P[k].grad)


@pytest.mark.parametrize("case", LOSS_CASES)
def test_r2u_oracle_loss_cases(case):
    z = np.load(R.__file__.replace("_r2u_oracle.py", "golden/r2u_loss_small.npz"))
    ign = int(z[f"{case}/ignore"])
    ign = None if ign < 0 else ign
    lg = torch.from_numpy(z[f"{case}/logits"]).double().requires_grad_(True)
    loss, dice = R.dice_loss(lg, torch.from_numpy(z[f"{case}/labels"]), ign)
    loss.backward()
    assert math.isclose(float(loss.detach()), float(z[f"{case}/loss"]), rel_tol=1e-12, abs_tol=1e-15)
    assert math.isclose(float(dice), float(z[f"{case}/dice"]), rel_tol=1e-12, abs_tol=1e-15)
    ref = z[f"{case}/dlogits"]
    np.testing.assert_allclose(lg.grad.numpy(), ref, rtol=1e-9, atol=1e-15)
    if case == "c":
        assert float(loss.detach()) == 0.0 and not ref.any()
    # fp32: the module's own arithmetic
    l32, d32 = R.dice_loss(torch.from_numpy(z[f"{case}/logits"]),
                           torch.from_numpy(z[f"{case}/labels"]), ign)
    assert math.isclose(float(l32), float(z[f"{case}/loss32"]), rel_tol=1e-5, abs_tol=1e-12)
    assert math.isclose(float(d32), float(z[f"{case}/dice32"]), rel_tol=1e-5, abs_tol=1e-12)


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_r2u_layouts_match_reference_state_dict(name):
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
    plan = E.R2UPlan(batch=1, in_ch=meta["in_ch"], depth=16, height=32, width=32,
                     num_classes=meta["K"], base=meta["base"], t=meta["t"])
    assert [(n, s) for n, s, _o, _k in plan.params] == named
    assert len(plan.params) == 73
    offs = [o for _n, _s, o, _k in plan.params]
    assert offs == sorted(offs) and len(set(offs)) == len(offs)
    assert plan.nfloats == sum(int(np.prod(s)) for _n, s in named)
    assert plan.nfloats == offs[-1] + plan.params[-1][3] and plan.ws_bytes > 0


def test_r2u_registry_entry(monkeypatch):
    from innovative3D import config as C
    import innovative3D.models as M
    assert C.VARIANT_NAMES[-1] == "R2UNet3D" and C.VARIANT_NAMES[-2] == "SwinUNETR"
    name, factory, dm, ck = C.variant("R2UNet3D")
    lit = factory()
    assert isinstance(lit, M.LitR2UNet3D_Published) and callable(dm)
    want = load("r2u_registry_k13")["meta"]["hparams"]
    assert {k: lit.hparams[k] for k in want} == want and set(lit.hparams) == set(want)
    assert lit.backbone.out_ch == 16 and lit.backbone.e1.ru.t == 2
    opt = lit.configure_optimizers()
    assert type(opt) is torch.optim.Adam
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"]) == (1e-3, 0.0)
    assert ck.name == "R2UNet3D"
    monkeypatch.setenv("INNOVATIVE3D_VARIANT", "R2UNet3D")
    assert [v[0] for v in C.selected_variants()] == ["R2UNet3D"]


def test_r2u_plan_rejects_bad_arguments():
    from innovative3D import _engine as E
    ok = dict(batch=1, in_ch=1, depth=16, height=32, width=32, num_classes=13, base=16, t=2)
    E.R2UPlan(**ok)
    with pytest.raises(E.SpffError, match="multiples of 16"):
        E.R2UPlan(**{**ok, "height": 24})
    for bad in ({"base": 12}, {"t": 0}, {"num_classes": 1}, {"num_classes": 33}, {"in_ch": 9},
                {"depth": 5}):
        with pytest.raises(E.SpffError):
            E.R2UPlan(**{**ok, **bad})
    E.R2UPlan(**{**ok, "num_classes": 32, "base": 24, "t": 3, "in_ch": 8})


def test_r2u_runs_only_on_device():
    import innovative3D.models as M
    from innovative3D import _engine as E
    m = M.LitR2UNet3D_Published(num_classes=3, base_features=8)
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 16, 16, 32))
    with pytest.raises(E.SpffError, match="no CPU fallback"):
        m._dice_only_loss_with_logits(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 2, 4, 4).long())


def test_r2u_binary_branch_is_refused():
    import innovative3D.models as M
    with pytest.raises(NotImplementedError, match="num_classes == 1"):
        M.LitR2UNet3D_Published(num_classes=1)


def test_unified_loss_patches_r2u(capsys):
    import innovative3D.models as M
    from innovative3D.unified_loss import apply_unified_loss
    steps = ("training_step", "validation_step", "test_step")
    lits = [c for c in vars(M).values()
            if isinstance(c, type) and issubclass(c, M.pl.LightningModule)]
    saved = {c: {k: vars(c)[k] for k in steps if k in vars(c)} for c in lits}
    try:
        patched = apply_unified_loss()
        assert "LitR2UNet3D_Published" in patched
        assert M.LitR2UNet3D_Published.training_step.__module__ == "innovative3D.unified_loss"
        assert M.LitR2UNet3D_Published.test_step.__module__ == "innovative3D.unified_loss"
    finally:  # the classes as they were: own steps restored, added ones removed
        for c, own in saved.items():
            for k in steps:
                if k in own:
                    setattr(c, k, own[k])
                elif k in vars(c):
                    delattr(c, k)
