"""R2UNet3D variant on the HIP engine against the fixtures the reference itself produced
(tests/golden/r2u_*.npz).  Marked gpu.

Per fixture and conv arithmetic (f32, bf16x6, f16x3): logits within 1e-3 of the reference's
PyTorch-CPU forward, at most 8 argmax flips and every one at a reference near-tie (top-2 gap
< 2 x max|dlogit|), the Dice-only loss within 1e-5 relative, and every parameter gradient
against a kink-consistent fp64 oracle (tests/_r2u_oracle.py with the ReLU signs and max-pool
argmaxes the engine saw: an activation within fp32 rounding of 0 may take either side)
within max(1e-3, 8 x the fp32 oracle's own error) of max|g|.  The loss kernel alone
against the fp64 loss and dlogits of four small cases; determinism; the no-grad forward;
the H / W padding and crop."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _r2u_oracle as R
from _compare import (assert_no_grad_forward_equals_train, assert_steps_bitwise, cached_oracle,
                      check_grads_rows, check_logits, grad_errors, kink_hooks, ncdhw, track_plan)
from _golden import GOLDEN, load, synth_state_of
import innovative3D.models as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVEL = dict(zip(R.BLOCKS, (0, 1, 2, 3, 4, 3, 2, 1, 0)))


def cfg_of(meta):
    return R.R2UCfg(num_classes=meta["K"], base=meta["base"], in_ch=meta["in_ch"], t=meta["t"],
                    pad_multiple=meta["pad_multiple"])


def build(d, mth=None):
    meta = d["meta"]
    m = M.LitR2UNet3D_Published(num_classes=meta["K"], in_channels=meta["in_ch"],
                                base_features=meta["base"], t=meta["t"],
                                pad_multiple=meta["pad_multiple"],
                                ignore_index=meta["ignore_index"])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_of(d).items()},
                      strict=True)
    if mth is not None:
        m.math = mth
    return m.to(DEV)


def engine_hooks(m, t):
    """ReLU sign patterns and pool argmaxes as the engine saw them.  (A step k < t stores
    twice its ReLU output: the sign pattern is the same.)"""
    plan = m._last_plan
    c = plan.cfg
    masks, pidx = {}, {}
    for n in R.BLOCKS:
        l = LEVEL[n]
        dims = (c.batch, c.depth >> l, c.height >> l, c.width >> l)
        for s in [f"ru{k}" for k in range(1, t + 1)] + ["out"]:
            a = ncdhw(plan.saved(f"{n}.{s}").cpu(), *dims)
            masks[f"{n}.{s}"] = a > 0
        if n in ("e1", "e2", "e3", "e4"):
            e = ncdhw(plan.saved(f"{n}.out").cpu(), *dims)
            pidx[f"pool{l + 1}"] = F.max_pool3d(e, 2, return_indices=True)[1]
    return kink_hooks(masks, pidx)


def oracle_grads(name, d, hooks, digest):
    """(g64, g32): one oracle run per fixture and distinct branch set"""
    def run():
        out = []
        for dtype in (torch.float64, torch.float32):
            P = R.params_from_state(synth_state_of(d), dtype=dtype)
            R.fwd_bwd(P, torch.from_numpy(d["x"]).to(dtype), torch.from_numpy(d["labels"]),
                      cfg_of(d["meta"]), d["meta"]["ignore_index"], hooks)
            out.append({k: v.grad.detach().double().numpy() for k, v in P.items()})
        return tuple(out)
    return cached_oracle((name, digest), run)


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", ["r2u_registry_k13", "r2u_core_b8_t3"])
def test_r2unet_matches_reference(name, mth):
    d = load(name)
    meta = d["meta"]
    m = build(d, mth)
    track_plan(m)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    m.train()
    logits = m(x)
    loss, dice = m._dice_only_loss_with_logits(logits, y, ignore_index=meta["ignore_index"])
    loss.backward()
    torch.cuda.synchronize()
    lg = logits.detach().cpu().numpy()
    ref = d["logits"]
    err, nf, _flips = check_logits(f"{name}/{mth}", lg, ref, max_flips=8)
    loss = loss.detach()
    print(f"  loss {float(loss):.7f} vs {float(d['loss']):.7f}  dice {float(dice):.7f} vs "
          f"{float(d['dice']):.7f}")
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
    # gradients vs the kink-consistent fp64 oracle
    hooks, digest = engine_hooks(m, meta["t"])
    g64, g32 = oracle_grads(name, d, hooks, digest)
    named = dict(m.named_parameters())
    check_grads_rows(grad_errors({k: named[k].grad for k in g64}, g64, g32))
    if name != "r2u_registry_k13":
        return
    # train.py's path: apply_unified_loss() rebinds the steps to CE + 0.5 hard Dice.  Against
    # the reference's ce_plus_macro_dice_loss of its own logits: the CE mean moves by at most
    # 2 max|dlogit| (|dCE/dlogits|_1 <= 2 per voxel); the hard Dice moves only with an argmax
    # flip, each of which changes two classes' dice by at most 2 / (their label count), i.e.
    # the macro term (weight 0.5, mean over K) by at most 2 / (K min_count); 1e-5 relative for
    # the fp32 reductions.
    from innovative3D.unified_loss import apply_unified_loss
    steps = ("training_step", "validation_step", "test_step")
    lits = [c for c in vars(M).values() if isinstance(c, type) and issubclass(c, M.pl.LightningModule)]
    saved = {c: {k: vars(c)[k] for k in steps if k in vars(c)} for c in lits}
    try:
        apply_unified_loss()
        lu = float(m.training_step((x, y), 0))
    finally:
        for c, own in saved.items():
            for k in steps:
                if k in own:
                    setattr(c, k, own[k])
                elif k in vars(c):
                    delattr(c, k)
    ref_u = float(d["loss_unified"])
    lab = d["labels"]
    counts = np.bincount(lab[lab != 255].reshape(-1), minlength=meta["K"])
    bound = 2 * err + 1e-5 * abs(ref_u) + nf * 2.0 / (meta["K"] * max(1, counts[counts > 0].min()))
    print(f"  unified loss {lu:.7f} vs {ref_u:.7f} (bound {bound:.2e})")
    assert abs(lu - ref_u) <= bound


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_r2u_dice_loss_kernel(case):
    z = np.load(GOLDEN / "r2u_loss_small.npz")
    K = int(z[f"{case}/K"])
    ign = int(z[f"{case}/ignore"])
    ign = None if ign < 0 else ign
    lg_np, y_np, ref = z[f"{case}/logits"], z[f"{case}/labels"], z[f"{case}/dlogits"]
    lg = torch.from_numpy(lg_np).to(DEV).requires_grad_(True)
    loss, dice = M.LitR2UNet3D_Published._dice_only_loss_with_logits(
        lg, torch.from_numpy(y_np).to(DEV), ignore_index=ign)
    loss.backward()
    torch.cuda.synchronize()
    g = lg.grad.double().cpu().numpy()
    # the fp32 oracle's own dlogits error
    t32 = torch.from_numpy(lg_np).requires_grad_(True)
    l32, _ = R.dice_loss(t32, torch.from_numpy(y_np), ign)
    l32.backward()
    scale = float(np.abs(ref).max())
    e32 = float(np.abs(t32.grad.double().numpy() - ref).max()) / max(scale, 1e-300)
    e_gpu = float(np.abs(g - ref).max()) / max(scale, 1e-300)
    # floor: one fp32 rounding per exp, sum, divide and the K-term inner product
    tol = max(8 * e32, (3 * K + 8) * 2.0 ** -24)
    print(f"case {case}: loss {float(loss):.8f} vs {float(z[f'{case}/loss']):.8f}  dlogits gpu "
          f"{e_gpu:.2e} fp32-oracle {e32:.2e} tol {tol:.2e}")
    if case == "c":  # no sample has foreground
        assert float(loss) == 0.0 and float(dice) == 0.0
        assert not g.any()
        return
    assert math.isclose(float(loss), float(z[f"{case}/loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(z[f"{case}/dice"]), rel_tol=1e-5)
    assert float(np.abs(g - ref).max()) <= tol * scale


def _step(m, x, y, ign):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss, _ = m._dice_only_loss_with_logits(logits, y, ignore_index=ign)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_r2unet_step_is_deterministic():
    d = load("r2u_core_b8_t3")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    assert_steps_bitwise(lambda: _step(m, x, y, 255))


def test_r2unet_no_grad_forward_equals_train_forward():
    d = load("r2u_core_b8_t3")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    m.train()
    assert_no_grad_forward_equals_train(m, x, eval_mode=True)


def test_r2unet_pad_crop():
    d = load("r2u_pad_hw")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    with torch.no_grad():
        logits = m(x)
        loss, dice = m._dice_only_loss_with_logits(logits, y, ignore_index=255)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == d["logits"].shape == (1, 13, 5, 24, 40)
    check_logits("r2u_pad_hw", logits, d["logits"], max_flips=8)
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
