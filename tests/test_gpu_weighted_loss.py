"""The voxel-weighted 3DUNet loss and the nnU-Net Dice + CE loss on the HIP loss driver, through
the Lit wrapper / models.dice_ce_loss.  Marked gpu.

Per fixture case (tests/golden/unet3d_loss_small.npz, nnunet_loss_small.npz): loss, CE and
Dice within 1e-5 relative of the fp64 reference (the fp64 oracle of tests/_wloss_oracle.py
where the reference runs in fp32 only) and dlogits within 1e-6 + 1e-4 |ref| elementwise -- the
bars test_rupp_loss_kernel applies to the same two-pass arithmetic.  Then the sparse-annotation
property (a voxel of weight 0 gets an all-zero dlogits row), labels outside [0, K), bitwise
repeatability, and one whole training step of the 3DUNet Lit module with a dict batch."""
import math

import numpy as np
import pytest
import torch

import _wloss_oracle as O
from _golden import GOLDEN, load
import innovative3D.models as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["a", "b", "c", "d", "e"]


def _close(tag, got, ref):
    print(f"  {tag}: {got:.8f} vs {ref:.8f}")
    assert math.isclose(got, ref, rel_tol=1e-5), tag  # a NaN is close to nothing


def _check_dlogits(g, ref):
    g, ref = g.detach().double().cpu().numpy(), np.asarray(ref, np.float64)
    err = np.abs(g - ref)
    print(f"  max|ddlogits| {float(err.max()):.2e} (max|ref| {float(np.abs(ref).max()):.2e})")
    assert not bool((~(err <= 1e-6 + 1e-4 * np.abs(ref))).any())


def _reference(z, c, kind, labels=None, **over):
    """(loss, ce, dice, dlogits) in fp64: the fixture's where it has them and nothing is
    overridden, else the oracle's"""
    if labels is None and not over and int(z[f"{c}/has64"]):
        return (float(z[f"{c}/loss"]), float(z[f"{c}/ce"]), float(z[f"{c}/dice"]),
                z[f"{c}/dlogits"])
    lg, y, kw = O.fixture_case(z, c, kind == "unet3d")
    kw.update(over)
    y = y if labels is None else labels
    fn, gfn = (O.unet3d_loss, O.unet3d_dlogits) if kind == "unet3d" else \
        (O.nnunet_loss, O.nnunet_dlogits)
    loss, ce, dice, _n = fn(lg.double(), y, **kw)
    return float(loss), float(ce), float(dice), gfn(lg.double(), y, **kw).numpy()


def _unet3d(z, c, labels=None, **over):
    """the Lit wrapper's combined loss on the device: (loss, out4, dlogits, voxel weights)"""
    lg, y, kw = O.fixture_case(z, c, True)
    kw.update(over)
    cw, vw = kw["class_weights"], kw["voxel_weights"]
    m = M.LitCicek3DUNet_DepthAdapter_Published(
        num_classes=lg.shape[1], ignore_index=kw["ignore_index"],
        class_weights=None if cw is None else cw.tolist(), voxel_weight_key="weight",
        ce_weight=kw["ce_weight"], dice_weight=kw["dice_weight"],
        include_bg_in_dice=kw["include_bg"])
    y = (y if labels is None else labels).to(DEV)
    t = lg.to(DEV).requires_grad_(True)
    loss, out4 = m._device_loss(t, y, None if vw is None else vw.to(DEV), m.ce_weight,
                                m.dice_weight)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), out4, t.grad, vw


def _nnunet(z, c, labels=None):
    lg, y, kw = O.fixture_case(z, c)
    y = (y if labels is None else labels).to(DEV)
    K = lg.shape[1]
    t = lg.to(DEV).requires_grad_(True)
    loss = M.dice_ce_loss(t, y, K, ignore_index=kw["ignore_index"], ce_weight=kw["ce_weight"],
                          dice_weight=kw["dice_weight"], include_background=kw["include_bg"])
    loss.backward()
    with torch.no_grad():
        ce = M.dice_ce_loss(t, y, K, ignore_index=kw["ignore_index"], ce_weight=1.0,
                            dice_weight=0.0, include_background=kw["include_bg"])
        dice = 1.0 - M.soft_dice_loss_from_logits(t, y, K, ignore_index=kw["ignore_index"],
                                                  include_background=kw["include_bg"])
    torch.cuda.synchronize()
    return loss.detach(), float(ce), float(dice), t.grad


@pytest.mark.parametrize("case", CASES)
def test_unet3d_loss_kernel(case):
    z = np.load(GOLDEN / "unet3d_loss_small.npz")
    loss, out4, g, _vw = _unet3d(z, case)
    rl, rc, rd, rg = _reference(z, case, "unet3d")
    _close("loss", float(loss), rl)
    _close("ce", float(out4[0]), rc)
    _close("dice", float(out4[2]), rd)
    _check_dlogits(g, rg)


@pytest.mark.parametrize("case", CASES)
def test_nnunet_loss_kernel(case):
    z = np.load(GOLDEN / "nnunet_loss_small.npz")
    loss, ce, dice, g = _nnunet(z, case)
    rl, rc, rd, rg = _reference(z, case, "nnunet")
    _close("loss", float(loss), rl)
    _close("ce", ce, rc)
    _close("dice", dice, rd)
    _check_dlogits(g, rg)


def test_zero_weight_voxels_get_no_gradient():
    """Sparse annotation: with the CE alone, a voxel of weight 0 has an all-zero dlogits row."""
    z = np.load(GOLDEN / "unet3d_loss_small.npz")
    _loss, _out4, g, vw = _unet3d(z, "a", dice_weight=0.0)
    rows = g.movedim(1, -1)[vw.to(DEV) == 0]
    assert rows.shape[0] > 50 and not bool(rows.any())
    assert bool(g.movedim(1, -1)[vw.to(DEV) > 0].any())


def _bad_labels(y, K):
    bad = y.clone()
    idx = torch.arange(0, y.numel(), 37)
    bad.view(-1)[idx[::2]] = K
    bad.view(-1)[idx[1::2]] = -3
    return bad, idx


@pytest.mark.parametrize("kind", ["unet3d", "nnunet"])
def test_out_of_range_labels_are_ignored(kind):
    z = np.load(GOLDEN / f"{kind}_loss_small.npz")
    K = int(z["a/K"])
    bad, idx = _bad_labels(torch.from_numpy(z["a/labels"]), K)
    if kind == "unet3d":
        loss, _out4, g, _vw = _unet3d(z, "a", labels=bad)
    else:
        loss, _ce, _dice, g = _nnunet(z, "a", labels=bad)
    rl, _rc, _rd, rg = _reference(z, "a", kind, labels=bad)
    assert math.isfinite(float(loss))
    _close("loss", float(loss), rl)
    _check_dlogits(g, rg)
    assert not bool(g.movedim(1, -1).reshape(-1, K)[idx.to(DEV)].any())


@pytest.mark.parametrize("kind", ["unet3d", "nnunet"])
def test_weighted_losses_are_deterministic(kind):
    z = np.load(GOLDEN / f"{kind}_loss_small.npz")
    run, ig = ((lambda: _unet3d(z, "a")), 2) if kind == "unet3d" else ((lambda: _nnunet(z, "a")), 3)
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[ig], b[ig])


def test_unet3d_lit_step_with_voxel_weights():
    """One training step at the fxu3d_core_b8 shape with a dict batch: the returned loss is the
    oracle's on the module's own logits, every parameter gradient is finite, and the logged
    keys are those of the unweighted path."""
    from innovative3D.weightgen import synth_state
    d = load("fxu3d_core_b8")
    K = d["meta"]["K"]
    m = M.LitCicek3DUNet_DepthAdapter_Published(num_classes=K, voxel_weight_key="weight",
                                                dice_weight=0.3)
    st = synth_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=10)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    m = m.to(DEV).train()
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    rng = np.random.default_rng(7)
    w = (rng.random(y.shape) + 0.25).astype(np.float32)
    w[rng.random(y.shape) < 0.3] = 0.0
    w = torch.from_numpy(w)
    seen, fwd = {}, m.forward

    def capture(inp):
        seen["logits"] = fwd(inp)
        return seen["logits"]
    m.forward = capture
    keys = []
    m.log = lambda name, value, *a, **k: keys.append(name)
    loss = m.training_step({"image": x.to(DEV), "label": y.to(DEV), "weight": w.to(DEV)}, 0)
    loss.backward()
    torch.cuda.synchronize()
    ref = O.unet3d_loss(seen["logits"].detach().double().cpu(), y, ignore_index=255,
                        voxel_weights=w, ce_weight=1.0, dice_weight=0.3)[0]
    _close("loss", float(loss.detach()), float(ref))
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert keys == ["train_loss", "train_macro_dice"]
