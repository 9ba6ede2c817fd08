"""SwinUNETR variant (BASELINE config 5) on the HIP engine vs the CPU oracle
(oracle/swin_oracle.py, MONAI 1.5.2 semantics restated).  PARITY UNPINNED:
MONAI is absent offline and the reference holds no fixture for this model, so
the oracle itself is pinned only by its own CPU tests (tests/test_swin_cpu.py).

Tolerances: logits within 1e-3 of the fp64 oracle (the north star's bar) and
identical argmax outside near-ties; loss within 1e-5 relative; every parameter
gradient within max(1e-3, 16 x the fp32 oracle's error) of max|g| per tensor,
against a kink-consistent oracle: the residual blocks' LeakyReLUs take the
engine's own sign pattern (its saved a1 / out tensors), since an input within
fp32 rounding of the kink may legitimately take either slope (1 vs 0.01)."""
import math

import numpy as np
import pytest
import torch

from _compare import check_grads_rows, check_logits, grad_errors
from _swin_checks import engine_act_masks
from oracle import swin_oracle as S
from innovative3D.weightgen import synth_state
import innovative3D.models as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(B, D, H, W, K, seed):
    cfg = S.SwinCfg(num_classes=K)
    shp = S.param_shapes(cfg)
    st = synth_state(list(shp.items()), seed=seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, D, H, W, generator=g)
    y = torch.randint(0, K, (B, D, H, W), generator=g)
    y[torch.rand(B, D, H, W, generator=g) < 0.02] = 255
    return cfg, st, x, y


def _engine_model(st, K, mth):
    m = M.SwinUNETR(in_channels=1, out_channels=K, feature_size=12, depths=(1, 1, 1, 1),
                    num_heads=(1, 2, 4, 8), mlp_ratio=2.0)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in st.items()})
    m.load_state_dict(sd, strict=True)
    m.math = mth
    return m.to(DEV)


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("shape", [(2, 32, 64, 32), (1, 64, 64, 64), (1, 32, 32, 64)])
def test_swin_matches_oracle(shape, mth):
    B, D, H, W = shape
    K = 9
    cfg, st, x, y = _case(B, D, H, W, K, seed=3)
    m = _engine_model(st, K, mth)
    logits = m(x.to(DEV))
    loss = M._SwinLoss.apply(logits, y.to(DEV), K, 255, False, 0.5)
    loss.backward()
    torch.cuda.synchronize()
    lg = logits.detach().cpu().double()
    ref = {}
    S.ACT_MASKS = engine_act_masks(m, x.shape)
    try:
        for dt in (torch.float64, torch.float32):
            P = S.params_from_state(st, dtype=dt)
            rl, rloss = S.fwd_bwd(P, x, y, cfg)
            ref[dt] = (rl, rloss, {k: v.grad.double() for k, v in P.items()})
    finally:
        S.ACT_MASKS = None
    r64 = ref[torch.float64]
    check_logits(f"{shape}/{mth}", lg, r64[0])
    print(f"  loss {float(loss):.7f} vs {float(r64[1]):.7f}")
    assert abs(float(loss) - float(r64[1])) <= 1e-5 * abs(float(r64[1]))
    named = dict(m.named_parameters())
    rows = grad_errors({k: named[k].grad for k in r64[2]}, r64[2], ref[torch.float32][2])
    check_grads_rows(rows, factor=16, top=8, width=60)


# (K, B, (D, H, W), fraction of voxels at 255, include_bg, ce_weight, classes drawn)
LOSS_CASES = {
    "a": (13, 2, (3, 5, 7), 0.1, False, 0.5, 13),  # the registry setting; a partial last group
    "b": (3, 2, (2, 8, 9), 0.0, True, 0.3, 3),     # 64 % K != 0: idle column lanes; none ignored
    "c": (32, 1, (1, 9, 9), 0.1, False, 0.5, 32),  # the largest K: two row sets per wave
    "d": (5, 2, (4, 4, 5), 0.1, True, 0.5, 3),     # classes 3, 4 in no label; a 16-voxel tail
}


def loss_case(case):
    """(logits [B, K, D, H, W] of scale 3, labels, K, include_bg, ce_weight) on the CPU"""
    K, B, dhw, p_ign, include_bg, w, kdraw = LOSS_CASES[case]
    g = torch.Generator().manual_seed(11 + ord(case))
    lg = 3.0 * torch.randn(B, K, *dhw, generator=g)
    y = torch.randint(0, kdraw, (B, *dhw), generator=g)
    y[torch.rand(B, *dhw, generator=g) < p_ign] = 255
    assert (y != 255).any() and bool((y == 255).any()) == (p_ign > 0)
    return lg, y, K, include_bg, w


@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_swin_loss_kernel(case):
    """The soft-Dice + CE loss kernels alone (M._SwinLoss forward + backward) against
    oracle.swin_oracle.lit_loss in fp64: loss within 1e-5 relative, dlogits within
    max(8 x the fp32 oracle's own error, (3K + 8) 2^-24) of max|dlogits| (one fp32 rounding
    per exp, sum, divide and the K-term inner product), as test_r2u_dice_loss_kernel."""
    lg, y, K, include_bg, w = loss_case(case)
    cfg = S.SwinCfg(num_classes=K, ce_weight=w, include_bg_in_dice=include_bg, ignore_index=255)
    ref = {}
    for dt in (torch.float64, torch.float32):
        t = lg.to(dt, copy=True).requires_grad_(True)
        loss = S.lit_loss(t, y, cfg)
        loss.backward()
        ref[dt] = (float(loss.detach()), t.grad.double().numpy())
    r_loss, r_dl = ref[torch.float64]
    x = lg.to(DEV).requires_grad_(True)
    loss = M._SwinLoss.apply(x, y.to(DEV), K, 255, include_bg, w)
    loss.backward()
    torch.cuda.synchronize()
    dl = x.grad.double().cpu().numpy()
    scale = float(np.abs(r_dl).max())
    e32 = float(np.abs(ref[torch.float32][1] - r_dl).max()) / scale
    e_gpu = float(np.abs(dl - r_dl).max()) / scale
    tol = max(8 * e32, (3 * K + 8) * 2.0 ** -24)
    loss = float(loss.detach())
    print(f"case {case}: loss {loss:.8f} vs {r_loss:.8f}  dlogits gpu {e_gpu:.2e} "
          f"fp32-oracle {e32:.2e} tol {tol:.2e}")
    assert math.isclose(loss, r_loss, rel_tol=1e-5)
    assert float(np.abs(dl - r_dl).max()) <= tol * scale


def test_swin_registry_forward_pads_to_32():
    """LitSwinUNETR_Published pads (replicate, centred) to a multiple of 32 and crops
    back (models.py:898-904): the registry layout [B, 1, 5, H, W]."""
    from innovative3D.config import variant
    lit = variant("SwinUNETR")[1]().to(DEV)
    x = torch.randn(1, 1, 5, 64, 64, device=DEV)
    with torch.no_grad():
        out = lit(x)
    assert tuple(out.shape) == (1, 13, 5, 64, 64)
    assert torch.isfinite(out).all()
