"""The shared autograd base of the device losses (helpers._DeviceLoss) and its five
subclasses, on the CPU: the engine calls are replaced by stubs that return a known dlogits,
so only the autograd plumbing runs -- layout, one-shot hand-out of dlogits, gradient arity."""
import pytest
import torch

import innovative3D._engine as E
import innovative3D.helpers as Hh
import innovative3D.models as M

B, K, D, H, W = 2, 3, 2, 3, 4


@pytest.fixture
def stub_engine(monkeypatch):
    """every loss entry returns out4 = [1, 2, 3, 4], dlogits_cl = 0, 1, 2, ... and (the CE
    pair) a conf matrix; scale_ multiplies in place on the CPU"""
    def outs(lcl, conf):
        assert lcl.shape[-1] == K and lcl.is_contiguous()
        out4 = torch.tensor([1.0, 2.0, 3.0, 4.0])
        dl = torch.arange(lcl.numel(), dtype=torch.float32).view(lcl.shape)
        return (out4, dl, torch.zeros(K, K + 1, dtype=torch.int64)) if conf else (out4, dl)

    for name, conf in (("ce_dice_forward", True), ("weighted_ce_forward", True),
                       ("swin_loss_forward", False), ("r2u_dice_loss_forward", False),
                       ("rupp_loss_forward", False)):
        monkeypatch.setattr(E, name, lambda lcl, labels, *a, _c=conf: outs(lcl, _c))
    monkeypatch.setattr(E, "scale_", lambda x, s: x.mul_(s))


# (Function, arguments after (logits, labels), number of outputs, index of the loss in out4)
LOSSES = {
    "_CEDice": (Hh._CEDice, (K, 255, 1e-6, None), 3, 1),
    "_WeightedCE": (M._WeightedCE, (K, 255, torch.ones(K)), 2, 0),
    "_SwinLoss": (M._SwinLoss, (K, 255, False, 0.5), 1, 1),
    "_R2UDiceLoss": (M._R2UDiceLoss, (K, None), 2, 1),
    "_RUPPLoss": (M._RUPPLoss, (K, 255, False, 0.5, 0.5), 2, 1),
}


@pytest.mark.parametrize("name", sorted(LOSSES))
@pytest.mark.parametrize("ndim", [5, 4])
def test_device_loss_gradients_and_second_backward(stub_engine, name, ndim):
    fn, args, nout, iloss = LOSSES[name]
    assert issubclass(fn, Hh._DeviceLoss)
    shape = (B, K, D, H, W) if ndim == 5 else (B, K, H, W)
    logits = torch.zeros(shape, requires_grad=True)
    labels = torch.zeros(shape[:1] + shape[2:], dtype=torch.int64)
    out = fn.apply(logits, labels, *args)
    out = out if isinstance(out, tuple) else (out,)
    assert len(out) == nout
    loss = out[0]
    assert float(loss.detach()) == [1.0, 2.0, 3.0, 4.0][iloss]
    assert loss.requires_grad and not any(o.requires_grad for o in out[1:])
    # one gradient per input, or autograd raises; dlogits scaled by the incoming gradient and
    # back in the logits' layout
    (2.0 * loss).backward(retain_graph=True)
    cl = (B, 1, H, W, K) if ndim == 4 else (B, D, H, W, K)
    n = B * K * H * W * (D if ndim == 5 else 1)
    want = 2.0 * torch.arange(n, dtype=torch.float32).view(cl).permute(0, 4, 1, 2, 3)
    assert torch.equal(logits.grad, want.reshape(shape))
    with pytest.raises(RuntimeError, match="backward ran twice through the same graph"):
        loss.backward(retain_graph=True)
