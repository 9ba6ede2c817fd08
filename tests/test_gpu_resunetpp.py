"""ResUNet++ variant on the HIP engine against the fixtures the reference itself produced
(tests/golden/rupp_*.npz).  Marked gpu.

Per fixture and conv arithmetic (f32, bf16x6, f16x3): logits within 1e-3 of the reference's
PyTorch-CPU forward, at most 8 argmax flips and every one at a reference near-tie (top-2 gap
< 2 x max|dlogit|), loss, dice and CE within 1e-5 relative, and every parameter gradient
against a kink-consistent fp64 oracle (tests/_rupp_oracle.py with the ReLU signs and max-pool
argmaxes the engine saw: an activation within fp32 rounding of 0 may take either side)
within max(1e-3, 8 x the fp32 oracle's own error) of max|g|.  The dilated conv alone through
the op-level ABI against an fp64 conv; the loss kernels alone against the fp64 loss and
dlogits of five small cases; determinism; the no-grad forward; the H / W padding and crop."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rupp_oracle as R
from _compare import (assert_no_grad_forward_equals_train, assert_steps_bitwise, cached_oracle,
                      check_grads_rows, check_logits, grad_errors, kink_hooks, ncdhw, track_plan)
from _golden import GOLDEN, load, synth_state_of
import innovative3D.models as M
from innovative3D import _engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
AGS = {"ag4": 3, "ag3": 2, "ag2": 1}


def cfg_of(meta):
    return R.RUPPCfg(num_classes=meta["K"], base=meta["base"], in_ch=meta["in_ch"],
                     pad_multiple=meta["pad_multiple"])


def build(d, mth=None):
    meta = d["meta"]
    m = M.LitResUNetPP3D_Published(num_classes=meta["K"], in_channels=meta["in_ch"],
                                   base_features=meta["base"], pad_multiple=meta["pad_multiple"],
                                   ignore_index=meta["ignore_index"])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_of(d).items()},
                      strict=True)
    if mth is not None:
        m.math = mth
    return m.to(DEV)


def engine_hooks(m):
    """ReLU sign patterns and pool argmaxes as the engine saw them."""
    plan = m._last_plan
    c = plan.cfg
    masks, pidx = {}, {}

    def dims(l):
        return (c.batch, c.depth >> l, c.height >> l, c.width >> l)
    for n in R.UNITS:
        for s in ("a1", "out"):
            masks[f"{n}.{s}"] = ncdhw(plan.saved(f"{n}.{s}").cpu(), *dims(R.LEVEL[n])) > 0
        if n in ("e1", "e2", "e3", "e4"):
            e = ncdhw(plan.saved(f"{n}.out").cpu(), *dims(R.LEVEL[n]))
            pidx[f"pool{R.LEVEL[n] + 1}"] = F.max_pool3d(e, 2, return_indices=True)[1]
    masks["b_aspp.out"] = ncdhw(plan.saved("b_aspp.out").cpu(), *dims(4)) > 0
    for n, l in AGS.items():
        masks[f"{n}.att"] = ncdhw(plan.saved(f"{n}.att").cpu(), *dims(l)) > 0
    return kink_hooks(masks, pidx)


def oracle_grads(name, d, hooks, digest):
    """(g64, g32): one oracle run per fixture and distinct branch set"""
    def run():
        out = []
        torch.set_num_threads(8)
        for dtype in (torch.float64, torch.float32):
            P = R.params_from_state(synth_state_of(d), dtype=dtype)
            R.fwd_bwd(P, torch.from_numpy(d["x"]).to(dtype), torch.from_numpy(d["labels"]),
                      cfg_of(d["meta"]), d["meta"]["ignore_index"], hooks)
            out.append({k: v.grad.detach().double().numpy() for k, v in P.items()})
        return tuple(out)
    return cached_oracle((name, digest), run)


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", ["rupp_registry_k13", "rupp_core_b8", "rupp_aspp_wide"])
def test_resunetpp_matches_reference(name, mth):
    d = load(name)
    m = build(d, mth)
    track_plan(m)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    m.train()
    logits = m(x)
    loss, dice, ce = m._loss(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    lg = logits.detach().cpu().numpy()
    check_logits(f"{name}/{mth}", lg, d["logits"], max_flips=8)
    print(f"  loss {float(loss):.7f} vs {float(d['loss']):.7f}  dice {float(dice):.7f} vs "
          f"{float(d['dice']):.7f}  ce {float(ce):.7f} vs {float(d['ce']):.7f}")
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
    assert math.isclose(float(ce), float(d["ce"]), rel_tol=1e-5)
    # gradients vs the kink-consistent fp64 oracle
    hooks, digest = engine_hooks(m)
    g64, g32 = oracle_grads(name, d, hooks, digest)
    named = dict(m.named_parameters())
    assert set(named) == set(g64)
    check_grads_rows(grad_errors({k: named[k].grad for k in g64}, g64, g32), width=40)


def test_resunetpp_pad_crop():
    d = load("rupp_pad_hw")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    with torch.no_grad():
        logits = m(x)
        loss, dice, ce = m._loss(logits, y)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == d["logits"].shape == (1, 13, 5, 24, 40)
    check_logits("rupp_pad_hw", logits, d["logits"], max_flips=8)
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(d["dice"]), rel_tol=1e-5)
    assert math.isclose(float(ce), float(d["ce"]), rel_tol=1e-5)


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


DIL_CASES = [
    # B, D, H, W, cin, cout, wide (the output is a channel range of a 4 cout row)
    (2, 3, 5, 19, 16, 24, False),  # r = 4, 8 read only padding in D and H, not in W
    (1, 9, 17, 9, 40, 8, False),   # r = 8 reaches inside in D and H
    (1, 1, 2, 2, 8, 8, False),     # only the centre tap survives
    (1, 2, 6, 11, 8, 16, True),    # ldy = 4 cout, channel offset cout
]


@pytest.mark.parametrize("r", [1, 2, 4, 8])
@pytest.mark.parametrize("case", DIL_CASES)
def test_dilated_conv(case, r):
    """fwd / dgrad / wgrad of the dilated 3x3x3 conv against F.conv3d(dilation = padding = r)
    in fp64, at the tolerance of the fp32 conv checks of test_gpu_ops.py."""
    B, D, H, W, cin, cout, wide = case
    g = torch.Generator().manual_seed(11 + r)
    x = torch.randn(B, cin, D, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(cin * 27)
    dy = torch.randn(B, cout, D, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y64 = F.conv3d(xr, wr, None, padding=r, dilation=r)
    y64.backward(dy.double())
    ldy, off = (4 * cout, cout) if wide else (cout, 0)
    xcl, wd = _cl(x).to(DEV), w.to(DEV)
    dyrow = torch.full((B, D, H, W, ldy), 7.0)
    dyrow[..., off:off + cout] = _cl(dy)
    dyrow = dyrow.to(DEV)
    yrow = torch.full((B, D, H, W, ldy), -3.0, device=DEV)
    L, p, st = E.lib(), E._ptr, E._stream(torch.device(DEV))
    ws = torch.empty(L.spff_conv3d_dil_ws_bytes(cin, cout), dtype=torch.uint8, device=DEV)
    fo = 4 * off  # byte offset of the channel range
    E.check(L.spff_conv3d_dil_fwd(p(xcl), cin, p(wd), yrow.data_ptr() + fo, ldy, B, D, H, W, cin,
                                  cout, r, p(ws), st), "dil fwd")
    dxg = torch.empty(B, D, H, W, cin, device=DEV)
    E.check(L.spff_conv3d_dil_dgrad(dyrow.data_ptr() + fo, ldy, p(wd), p(dxg), cin, B, D, H, W,
                                    cin, cout, r, 0, p(ws), st), "dil dgrad")
    dx2 = dxg.clone()
    E.check(L.spff_conv3d_dil_dgrad(dyrow.data_ptr() + fo, ldy, p(wd), p(dx2), cin, B, D, H, W,
                                    cin, cout, r, 1, p(ws), st), "dil dgrad acc")
    dwg = torch.full_like(wd, 5.0)
    E.check(L.spff_conv3d_dil_wgrad(p(xcl), cin, dyrow.data_ptr() + fo, ldy, p(dwg), B, D, H, W,
                                    cin, cout, r, p(ws), st), "dil wgrad")
    torch.cuda.synchronize()
    yrow = yrow.cpu()
    if wide:  # the neighbouring channel ranges are untouched
        assert bool((yrow[..., :off] == -3.0).all()) and bool((yrow[..., off + cout:] == -3.0).all())
    for tag, got, ref in (("fwd", yrow[..., off:off + cout].double(), _cl(y64.detach())),
                          ("dgrad", dxg.cpu().double(), _cl(xr.grad)),
                          ("dgrad acc", dx2.cpu().double(), 2 * _cl(xr.grad)),
                          ("wgrad", dwg.cpu().double(), wr.grad)):
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"dil {case} r={r} {tag}: max err {err:.2e} (max|ref| {scale:.2e})")
        assert err <= 2e-5 * scale + 1e-6, tag
    if r >= max(D, H, W):  # only the centre tap is live: every other tap's gradient is zero
        live = torch.zeros(27, dtype=torch.bool)
        live[13] = True
        assert not dwg.cpu().reshape(cout, cin, 27)[:, :, ~live].any()


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_rupp_loss_kernel(case):
    z = np.load(GOLDEN / "rupp_loss_small.npz")
    K = int(z[f"{case}/K"])
    ign = int(z[f"{case}/ignore"])
    ign = None if ign < 0 else ign
    lg_np, y_np, ref = z[f"{case}/logits"], z[f"{case}/labels"], z[f"{case}/dlogits"]
    m = M.LitResUNetPP3D_Published(num_classes=K, base_features=8, ignore_index=ign,
                                   include_bg_in_dice=bool(int(z[f"{case}/include_bg"])),
                                   ce_weight=float(z[f"{case}/ce_weight"]),
                                   dice_weight=float(z[f"{case}/dice_weight"]))
    lg = torch.from_numpy(lg_np).to(DEV).requires_grad_(True)
    loss, dice, ce = m._loss(lg, torch.from_numpy(y_np).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    g = lg.grad.double().cpu().numpy()
    err = np.abs(g - ref)
    print(f"case {case}: loss {float(loss):.8f} vs {float(z[f'{case}/loss']):.8f}  dice "
          f"{float(dice):.8f} vs {float(z[f'{case}/dice']):.8f}  ce {float(ce):.8f} vs "
          f"{float(z[f'{case}/ce']):.8f}  max|ddlogits| {float(err.max()):.2e}")
    assert math.isclose(float(loss), float(z[f"{case}/loss"]), rel_tol=1e-5)
    assert math.isclose(float(dice), float(z[f"{case}/dice"]), rel_tol=1e-5)
    assert math.isclose(float(ce), float(z[f"{case}/ce"]), rel_tol=1e-5)
    assert bool((err <= 1e-6 + 1e-4 * np.abs(ref)).all())


def _step(m, x, y):
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss, _d, _c = m._loss(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_resunetpp_step_is_deterministic():
    d = load("rupp_core_b8")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    assert_steps_bitwise(lambda: _step(m, x, y))


def test_resunetpp_no_grad_forward_equals_train_forward():
    d = load("rupp_core_b8")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    m.train()
    assert_no_grad_forward_equals_train(m, x, eval_mode=True)


def test_resunetpp_steps_log_the_reference_keys():
    d = load("rupp_registry_k13")
    m = build(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    logged = {}
    m.log = lambda k, v, **kw: logged.__setitem__(k, float(torch.as_tensor(v).detach()))
    loss = m.training_step((x, y), 0)
    assert loss.requires_grad
    with torch.no_grad():
        vloss = m.validation_step({"image": x, "label": y}, 0)
    torch.cuda.synchronize()
    assert sorted(logged) == ["train_loss", "train_macro_dice", "val_loss", "val_macro_dice"]
    assert math.isclose(logged["train_loss"], float(d["loss"]), rel_tol=1e-5)
    assert math.isclose(logged["train_macro_dice"], float(d["dice"]), rel_tol=1e-5)
    assert math.isclose(float(vloss), float(d["loss"]), rel_tol=1e-5)
    assert logged["val_macro_dice"] == logged["train_macro_dice"]
