"""The voxel-weighted 3DUNet loss and the nnU-Net Dice + CE loss on the CPU: the oracle
(tests/_wloss_oracle.py) against the fixtures the reference produced, its closed-form dlogits
against autograd, the Python plumbing with stubbed engine calls, and the two C entry points'
argument checks (no device is touched)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _wloss_oracle as O
from _golden import GOLDEN
import innovative3D._engine as E
import innovative3D.helpers as Hh
import innovative3D.models as M

CASES = ["a", "b", "c", "d", "e"]
KINDS = {"unet3d": ("unet3d_loss_small.npz", O.unet3d_loss, O.unet3d_dlogits, True),
         "nnunet": ("nnunet_loss_small.npz", O.nnunet_loss, O.nnunet_dlogits, False)}


def _oracle(kind, case, dtype):
    """(loss, ce, dice as the fixture stores it, autograd dlogits, closed-form dlogits, z)"""
    name, loss_fn, grad_fn, weights = KINDS[kind]
    z = np.load(GOLDEN / name)
    lg, y, kw = O.fixture_case(z, case, weights)
    t = lg.to(dtype).requires_grad_(True)
    loss, ce, dice, _n = loss_fn(t, y, **kw)
    loss.backward()
    with torch.no_grad():
        closed = grad_fn(t.detach(), y, **kw)
    return float(loss.detach()), float(ce.detach()), float(dice.detach()), t.grad, closed, z


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_oracle_matches_reference_fixture(kind, case):
    # fp64: round-off of the same formula; fp32: one CPU's fp32 result against another's
    # (scalars as test_resunetpp_cpu.py, dlogits as tests/_compare.check_fixture_grads)
    loss, ce, dice, g, _closed, z = _oracle(kind, case, torch.float32)
    assert math.isclose(loss, float(z[f"{case}/loss32"]), rel_tol=1e-5)
    assert math.isclose(ce, float(z[f"{case}/ce32"]), rel_tol=1e-5)
    assert math.isclose(dice, float(z[f"{case}/dice32"]), rel_tol=1e-5)
    ref = z[f"{case}/dlogits32"]
    err = float(np.abs(g.numpy() - ref).max())
    assert err <= 5e-4 * float(np.abs(ref).max())
    if int(z[f"{case}/has64"]):
        loss, ce, dice, g, _closed, z = _oracle(kind, case, torch.float64)
        assert math.isclose(loss, float(z[f"{case}/loss"]), rel_tol=1e-9)
        assert math.isclose(ce, float(z[f"{case}/ce"]), rel_tol=1e-9)
        assert math.isclose(dice, float(z[f"{case}/dice"]), rel_tol=1e-9)
        ref = z[f"{case}/dlogits"]
        assert float(np.abs(g.numpy() - ref).max()) <= 1e-9 * float(np.abs(ref).max())
    else:
        assert kind == "unet3d" and f"{case}/class_weights" in z.files


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_closed_form_dlogits_equal_autograd(kind, case):
    """The formulas the gradient pass implements: fp64 round-off of a few hundred terms."""
    _l, _c, _d, g, closed, _z = _oracle(kind, case, torch.float64)
    assert float((g - closed).abs().max()) <= 1e-12 * float(g.abs().max()) + 1e-15


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_oracle_masks_out_of_range_labels(kind):
    """A label outside [0, K) behaves as an ignored one: same loss as with ignore_index there."""
    name, loss_fn, grad_fn, weights = KINDS[kind]
    z = np.load(GOLDEN / name)
    lg, y, kw = O.fixture_case(z, "a", weights)
    K = lg.shape[1]
    bad, ign = y.clone(), y.clone()
    idx = torch.arange(0, y.numel(), 37)
    bad.view(-1)[idx[::2]] = K
    bad.view(-1)[idx[1::2]] = -3
    ign.view(-1)[idx] = kw["ignore_index"]
    a = loss_fn(lg.double(), bad, **kw)
    b = loss_fn(lg.double(), ign, **kw)
    assert all(float(p) == float(q) for p, q in zip(a, b))
    d = grad_fn(lg.double(), bad, **kw).movedim(1, -1).reshape(-1, K)
    assert not d[idx].any() and torch.isfinite(d).all()


# ------------------------------------------------------------------ plumbing --
B, K, D, H, W = 2, 3, 2, 3, 4


@pytest.fixture
def stub_engine(monkeypatch):
    """the loss entries return out4 = [1, 2, 3, 4] and dlogits_cl = 0, 1, 2, ... and record
    their arguments; scale_ multiplies in place on the CPU"""
    calls = []

    def make(name, conf):
        def f(lcl, labels, *a, **k):
            assert lcl.shape[-1] == K and lcl.is_contiguous()
            calls.append((name, labels, a, k))
            out4 = torch.tensor([1.0, 2.0, 3.0, 4.0])
            dl = torch.arange(lcl.numel(), dtype=torch.float32).view(lcl.shape)
            return (out4, dl, torch.zeros(K, K + 1, dtype=torch.int64)) if conf else (out4, dl)
        return f
    for name, conf in (("unet3d_loss_forward", False), ("nnunet_loss_forward", False),
                       ("weighted_ce_forward", True)):
        monkeypatch.setattr(E, name, make(name, conf))
    monkeypatch.setattr(E, "confusion", lambda lcl, labels, k, ign: (
        calls.append(("confusion", labels, (k, ign), {})),
        torch.zeros(K, K + 1, dtype=torch.int64))[1])
    monkeypatch.setattr(E, "scale_", lambda x, s: x.mul_(s))
    return calls


LOSSES = {
    "_UNet3DLoss": (lambda: M._UNet3DLoss, (K, 255, None, None, False, 1.0, 0.5)),
    "_NNUNetLoss": (lambda: M._NNUNetLoss, (K, -1, False, 1.0, 1.0)),
}


@pytest.mark.parametrize("name", sorted(LOSSES))
@pytest.mark.parametrize("ndim", [5, 4])
def test_device_loss_hands_out_dlogits_once(stub_engine, name, ndim):
    fn, args = LOSSES[name][0](), LOSSES[name][1]
    assert issubclass(fn, Hh._DeviceLoss)
    shape = (B, K, D, H, W) if ndim == 5 else (B, K, H, W)
    logits = torch.zeros(shape, requires_grad=True)
    labels = torch.zeros(shape[:1] + shape[2:], dtype=torch.int64)
    loss, out4 = fn.apply(logits, labels, *args)
    assert float(loss.detach()) == 2.0 and out4.tolist() == [1.0, 2.0, 3.0, 4.0]
    assert loss.requires_grad and not out4.requires_grad
    (2.0 * loss).backward(retain_graph=True)
    cl = (B, 1, H, W, K) if ndim == 4 else (B, D, H, W, K)
    n = B * K * H * W * (D if ndim == 5 else 1)
    want = 2.0 * torch.arange(n, dtype=torch.float32).view(cl).permute(0, 4, 1, 2, 3)
    assert torch.equal(logits.grad, want.reshape(shape))
    with pytest.raises(RuntimeError, match="backward ran twice through the same graph"):
        loss.backward(retain_graph=True)


def _lg_y():
    return (torch.zeros(B, K, D, H, W, requires_grad=True),
            torch.zeros(B, D, H, W, dtype=torch.int64))


def test_registry_entry_and_adapter_call_the_nnunet_loss(stub_engine):
    lg, y = _lg_y()
    for f in (Hh.LOSS_REGISTRY["dice_ce_nnunet"], Hh.dice_ce_loss_adapter):
        del stub_engine[:]
        loss = f(lg, y, K, 255)
        assert float(loss.detach()) == 2.0 and loss.requires_grad
        (name, _labels, a, _k), = stub_engine
        # (K, ignore_index, include_bg, ce_weight, dice_weight): dice_ce_loss's defaults
        assert name == "nnunet_loss_forward" and a == (K, 255, False, 1.0, 1.0)
    del stub_engine[:]
    M.dice_ce_loss(lg, y, K)
    assert stub_engine[0][2] == (K, -1, False, 1.0, 1.0)
    del stub_engine[:]
    M.soft_dice_loss_from_logits(lg, y, K, include_background=True)
    assert stub_engine[0][2] == (K, -1, True, 0.0, 1.0)
    with pytest.raises(NotImplementedError):
        M.soft_dice_loss_from_logits(lg, y, K, eps=1e-6)


def _lit(**kw):
    m = M.LitCicek3DUNet_DepthAdapter_Published(num_classes=K, **kw)
    lg, y = _lg_y()
    m.forward = lambda x: lg
    m.keys = []
    m.log = lambda name, value, *a, **k: m.keys.append(name)
    return m, lg, y


def test_unet3d_wrapper_passes_voxel_weights_on(stub_engine):
    m, lg, y = _lit(voxel_weight_key="weight", class_weights=[1.0, 2.0, 3.0], dice_weight=0.3,
                    ce_weight=0.7, include_bg_in_dice=True)
    w = torch.rand(B, 1, D, H, W)  # a size-1 channel dimension is squeezed
    loss = m.training_step({"image": torch.zeros(B, 1, D, H, W), "label": y, "weight": w}, 0)
    assert float(loss.detach()) == 2.0 and loss.requires_grad
    (name, _labels, a, _k), (cname, _l2, ca, _k2) = stub_engine
    assert name == "unet3d_loss_forward" and cname == "confusion" and ca == (K, 255)
    k_, ign, cw, vw, bg, cew, dw = a
    assert (k_, ign, bg, cew, dw) == (K, 255, True, 0.7, 0.3)
    assert torch.equal(cw, torch.tensor([1.0, 2.0, 3.0])) and torch.equal(vw, w[:, 0])
    assert m.keys == ["train_loss", "train_macro_dice"]
    # the methods of the reference's surface: each one call of the same driver
    del stub_engine[:]
    m._weighted_softmax_ce(lg, y, w)
    m._dice_loss(lg, y)
    assert [c[2][5:] for c in stub_engine] == [(1.0, 0.0), (0.0, 1.0)]
    assert stub_engine[1][2][3] is None
    # ignore_index None: no mask
    m2, lg2, y2 = _lit(ignore_index=None, dice_weight=1.0)
    del stub_engine[:]
    m2.training_step((torch.zeros(B, 1, D, H, W), y2), 0)
    assert stub_engine[0][0] == "unet3d_loss_forward" and stub_engine[0][2][1] is None


def test_unet3d_wrapper_list_batch_without_dice_stays_on_weighted_ce(stub_engine):
    m, _lg, y = _lit(voxel_weight_key="weight")
    loss = m.training_step((torch.zeros(B, 1, D, H, W), y), 0)
    assert float(loss.detach()) == 1.0  # _WeightedCE returns out4[0]
    assert [c[0] for c in stub_engine] == ["weighted_ce_forward"]
    assert m.keys == ["train_loss", "train_macro_dice"]


@pytest.mark.parametrize("shape", [(B, D, H), (B, 2, D, H, W), (1, D, H, W), (B, D, H, W, 1)])
def test_voxel_weights_of_a_wrong_shape_raise(stub_engine, shape):
    m, _lg, y = _lit(voxel_weight_key="weight")
    with pytest.raises(ValueError, match="voxel weights"):
        m.training_step({"image": torch.zeros(B, 1, D, H, W), "label": y,
                         "weight": torch.ones(shape)}, 0)
    assert not stub_engine


def test_focal_plus_gradient_still_raises_and_says_why():
    lg, y = _lg_y()
    with pytest.raises(NotImplementedError, match="IndexError"):
        Hh.LOSS_REGISTRY["focal_plus_gradient"](lg, y, K, 255)


# --------------------------------------------------------------------- C ABI --
@pytest.mark.parametrize("entry,tail", [
    ("spff_unet3d_loss", (1, 255, None, None, 0, 1.0, 0.5)),
    ("spff_nnunet_loss", (1, 255, 0, 1.0, 1.0)),
])
def test_loss_entries_reject_bad_arguments(entry, tail):
    L = E.lib()
    assert entry in E.EXPORTED and entry + "_ws_bytes" in E.EXPORTED
    fn = getattr(L, entry)
    buf = ctypes.create_string_buffer(64)  # never dereferenced: the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(batch, vps, k, out4=p, dl=p, ws=p):
        return fn(p, p, batch, vps, k, *tail, out4, dl, ws, None)
    for args in ((1, 8, 1), (1, 8, 33), (0, 8, 5), (1, 0, 5)):
        assert call(*args) == -1, args  # SPFF_EINVAL
    assert call(1, 8, 5, out4=None) == -1
    assert call(1, 8, 5, dl=None) == -1
    assert call(1, 8, 5, ws=None) == -1
    ws = getattr(L, entry + "_ws_bytes")
    n13, n5 = int(ws(2, 13)), int(ws(2, 5))
    assert 0 < n5 < n13
    # nq = 3 K + 2 (4 K + 2 with the squares) doubles per block partial and total
    assert n13 >= 2 * 257 * ((4 if "nnunet" in entry else 3) * 13 + 2) * 8
