"""The generation guard of the five variant plans (the main engine's is covered by
test_gpu_parity / test_gpu_memory).  Marked gpu.

One module per variant at its smallest valid shape, two forwards on it:
  * the backward of the first raises SpffError (in Python, before any launch): the plan keeps
    one forward's activations and the second forward overwrote them;
  * the backward of the second succeeds, and its gradients are bitwise those of a fresh
    module with the same weights doing one forward and one backward (every plan's
    accumulation order is fixed);
  * after E.release_workspace(plan) a pending backward raises instead of running on another
    workspace.

ResUNet++ runs at 1x1x16x16x32, not 16^3: its plan rejects a bottleneck of one voxel per
sample (InstanceNorm3d needs more than one), so 16x16x32 is its smallest valid volume.
"""
import copy

import pytest
import torch

import innovative3D.models as M
from innovative3D import _engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 3


def _r2u():
    return M.LitR2UNet3D_Published(num_classes=K, in_channels=1, base_features=8), (1, 1, 16, 16, 16)


def _rupp():
    return (M.LitResUNetPP3D_Published(num_classes=K, in_channels=1, base_features=8),
            (1, 1, 16, 16, 32))


def _unet3d():
    return M.Cicek3DUNet(num_classes=K, base=8, in_channels=1), (1, 1, 16, 16, 16)


def _swin():
    return (M.SwinUNETR(in_channels=1, out_channels=K, feature_size=4, depths=(1, 1, 1, 1),
                        num_heads=(1, 2, 4, 8), mlp_ratio=2.0), (1, 1, 32, 32, 64))


def _unetr():
    return (M.UNETR(in_channels=1, out_channels=K, img_size=(32, 32, 32), feature_size=8,
                    hidden_size=32, mlp_dim=64, num_heads=2), (1, 1, 32, 32, 32))


VARIANTS = {"R2UNet3D": _r2u, "ResUNet++": _rupp, "3DUNet": _unet3d, "SwinUNETR": _swin,
            "UNETR": _unetr}


def _grads(m):
    """{name: gradient}; None for a parameter outside the plan (UNETR registers some)"""
    return {n: None if p.grad is None else p.grad.detach().clone()
            for n, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_second_forward_invalidates_the_first_backward(name):
    torch.manual_seed(0)
    m, shape = VARIANTS[name]()
    m.train()
    fresh = copy.deepcopy(m)  # the same weights (and BatchNorm buffers), never run
    m, fresh = m.to(DEV), fresh.to(DEV)
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn(shape, generator=g).to(DEV)
    x2 = torch.randn(shape, generator=g).to(DEV)
    w = torch.randn((shape[0], K, *shape[2:]), generator=g).to(DEV)

    y1 = m(x1)
    y2 = m(x2)
    plan = y2.grad_fn.plan
    assert plan is y1.grad_fn.plan and plan.NAME == name
    with pytest.raises(E.SpffError, match="another forward ran"):
        (y1 * w).sum().backward()
    assert all(p.grad is None for p in m.parameters())  # nothing ran
    (y2 * w).sum().backward()

    yf = fresh(x2)
    (yf * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(y2, yf)
    got, ref = _grads(m), _grads(fresh)
    assert list(got) == list(ref) and sum(v is not None for v in got.values()) == len(plan.params)
    for n in got:
        assert (got[n] is None) == (ref[n] is None), n
        assert got[n] is None or torch.equal(got[n], ref[n]), n

    y3 = m(x1)
    E.release_workspace(plan)
    with pytest.raises(E.SpffError, match="another forward ran"):
        (y3 * w).sum().backward()
