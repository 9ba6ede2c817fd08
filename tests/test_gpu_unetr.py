"""UNETR variant on the HIP engine: the two new device ops against fp64 torch, the whole
network against the fixtures (tests/golden/unetr_*.npz) and the fp64 oracle
(tests/_unetr_oracle.py, MONAI 1.5.2 semantics restated -- PARITY UNPINNED: MONAI is absent
offline, so the fixtures pin the reference's pad / resample / crop / loss / gradient flow
around the restated body, not the body itself), and the plan's behaviour.

Op tolerances: 16 x the error that the same fp32 computation in torch on the CPU shows
against fp64 for that case, floored at 1e-6 of max|ref|; both figures are printed.
Network tolerances, as tests/test_gpu_swin.py: logits within 1e-3 of the reference logits
and no argmax difference outside near-ties (top1 - top2 < 2 x err); loss within 1e-5
relative; every gradient within max(1e-3, 16 x the fp32 oracle's error) of max|g|.  The two
small fixtures check the gradients against the kink-consistent fp64 oracle (the residual
blocks' LeakyReLUs take the engine's own sign pattern), the registry-width one against the
stored head / tail / sum."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _unetr_oracle as U
import innovative3D.models as M
from _compare import (assert_no_grad_forward_equals_train, assert_steps_bitwise, check_grads_rows,
                      check_logits, fp32_bound, grad_errors, lrelu_act_masks)
from _golden import load, synth_state_of
from innovative3D import _engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ attention --
def _attn_torch(qkv, B, nh):
    T, C3 = qkv.shape
    n, C = T // B, C3 // 3
    hd = C // nh
    q, k, v = qkv.reshape(B, n, 3, nh, hd).permute(2, 0, 3, 1, 4)
    att = torch.softmax((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1)
    return (att @ v).permute(0, 2, 1, 3).reshape(T, C)


@pytest.mark.parametrize("shape", [(1, 2, 64, 216), (2, 2, 64, 27), (1, 3, 16, 8), (1, 1, 32, 1),
                                   (1, 2, 64, 343)])
def test_vit_attention_matches_fp64(shape):
    B, nh, hd, n = shape
    g = torch.Generator().manual_seed(11 + n)
    qkv = torch.randn(B * n, 3 * nh * hd, generator=g)
    dO = torch.randn(B * n, nh * hd, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        a = qkv.clone().to(dt).requires_grad_(True)
        o = _attn_torch(a, B, nh)
        o.backward(dO.to(dt))
        res[dt] = (o.detach(), a.grad)
    O, lse = E.vit_attn_fwd(qkv.to(DEV), B, nh)
    dqkv = E.vit_attn_bwd(qkv.to(DEV), O, dO.to(DEV), lse, B, nh)
    torch.cuda.synchronize()
    for name, got, k in (("O", O, 0), ("dqkv", dqkv, 1)):
        ref = res[torch.float64][k]
        bound, e32, ref_max = fp32_bound(ref, res[torch.float32][k])
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[vit_attn {shape}] {name}: err {err:.3e}  cpu-fp32 err {e32:.3e}  "
              f"bound {bound:.3e}  max|ref| {ref_max:.3e}")
        assert err <= bound, (name, err, bound)
    # saved log-sum-exp
    T = B * n
    q, k, _ = qkv.double().reshape(B, n, 3, nh, hd).permute(2, 0, 3, 1, 4)
    ref_lse = torch.logsumexp((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1)
    assert float((lse.cpu().double() - ref_lse).abs().max()) <= 1e-5 * max(
        1.0, float(ref_lse.abs().max()))
    assert T == O.shape[0]


def test_vit_attention_is_deterministic():
    B, nh, hd, n = 2, 2, 64, 216
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * n, 3 * nh * hd, generator=g).to(DEV)
    dO = torch.randn(B * n, nh * hd, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        O, lse = E.vit_attn_fwd(qkv, B, nh)
        outs.append((O, lse, E.vit_attn_bwd(qkv, O, dO, lse, B, nh)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------- resample --
RESIZE = [((16, 80, 48), (48, 48, 48), 5), ((48, 48, 48), (16, 80, 48), 5),
          ((96, 96, 96), (16, 96, 64), 13)]


@pytest.mark.parametrize("src,dst,C", RESIZE)
def test_resize3d_matches_fp64(src, dst, C):
    B = 2 if C == 5 else 1
    g = torch.Generator().manual_seed(C + src[0])
    x = torch.randn(B, C, *src, generator=g)
    dy = torch.randn(B, C, *dst, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        a = x.clone().to(dt).requires_grad_(True)
        y = F.interpolate(a, size=dst, mode="trilinear", align_corners=False)
        y.backward(dy.to(dt))
        res[dt] = (y.detach(), a.grad)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    y = E.resize3d_fwd(cl(x).to(DEV), dst)
    dx = E.resize3d_bwd(cl(dy).to(DEV), src)
    torch.cuda.synchronize()
    for name, got, k in (("y", y, 0), ("dx", dx, 1)):
        ref = cl(res[torch.float64][k])
        bound, e32, ref_max = fp32_bound(ref, cl(res[torch.float32][k]))
        err = float((got.cpu().double() - ref).abs().max())
        print(f"[resize3d {src}->{dst} C={C}] {name}: err {err:.3e}  cpu-fp32 err {e32:.3e}  "
              f"bound {bound:.3e}  max|ref| {ref_max:.3e}")
        assert err <= bound, (name, err, bound)
    # <R x, y> = <x, R^T y>: both sides are sums of fp32 values that each carry a few
    # roundings (8 products and 7 sums per output, as many per adjoint term): 64 eps of the
    # sum of the absolute terms bounds the difference
    yd, dxd = y.cpu().double(), dx.cpu().double()
    lhs = float((yd * cl(dy).double()).sum())
    rhs = float((cl(x).double() * dxd).sum())
    scale = float((yd * cl(dy).double()).abs().sum())
    print(f"[resize3d {src}->{dst}] <Rx,y> {lhs:.9e}  <x,RTy> {rhs:.9e}  sum|terms| {scale:.3e}")
    assert abs(lhs - rhs) <= 64 * 2.0 ** -24 * scale


def test_resize3d_identity_axis_is_bit_exact():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 16, 80, 48, 5, generator=g).to(DEV)
    # every axis unchanged: the input comes back
    assert torch.equal(E.resize3d_fwd(x, (16, 80, 48)), x)
    assert torch.equal(E.resize3d_bwd(x, (16, 80, 48)), x)
    # W unchanged (48 -> 48): the same bits as resampling D and H with W folded into the
    # channels, where no W neighbour exists at all
    y = E.resize3d_fwd(x, (48, 48, 48))
    y2 = E.resize3d_fwd(x.reshape(1, 16, 80, 1, 48 * 5), (48, 48, 1)).reshape(1, 48, 48, 48, 5)
    assert torch.equal(y, y2)
    dy = torch.randn(1, 48, 48, 48, 5, generator=g).to(DEV)
    d1 = E.resize3d_bwd(dy, (16, 80, 48))
    d2 = E.resize3d_bwd(dy.reshape(1, 48, 48, 1, 48 * 5), (16, 80, 1)).reshape(1, 16, 80, 48, 5)
    assert torch.equal(d1, d2)


# ---------------------------------------------------------------- whole net --
RB_LEVEL = {"encoder1.layer": 0, "encoder2.blocks.0.1": 2, "encoder2.blocks.1.1": 1,
            "encoder3.blocks.0.1": 2, "decoder5.conv_block": 3, "decoder4.conv_block": 2,
            "decoder3.conv_block": 1, "decoder2.conv_block": 0}
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        d = load(name)
        d["state"] = synth_state_of(d)
        _FIX[name] = d
    return _FIX[name]


def _lit(d, mth):
    m = d["meta"]
    lit = M.LitUNETR_Published(num_classes=m["K"], img_size=tuple(m["img"]),
                               feature_size=m["feature_size"], hidden_size=m["hidden"],
                               mlp_dim=m["mlp_dim"], num_heads=m["heads"], ignore_index=255,
                               include_bg_in_dice=False, ce_weight=0.5)
    lit.load_state_dict({k: torch.from_numpy(v) for k, v in d["state"].items()}, strict=True)
    lit.net.net.math = mth
    return lit.to(DEV)


def _step(lit, d):
    lit.zero_grad(set_to_none=True)
    logits = lit(torch.from_numpy(d["x"]).to(DEV))
    loss = lit._loss(logits, torch.from_numpy(d["labels"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach()


def _engine_act_masks(lit, d):
    """Sign patterns of the residual blocks' LeakyReLU inputs as the engine saw them:
    sign(a1) and sign(out) (a LeakyReLU keeps the sign of its input)."""
    B, _c, D, H, W = d["x"].shape
    pad = [-(-v // 16) * 16 for v in (D, H, W)]
    plan = lit.net.net._plan(torch.empty((B, 1, *pad), device=DEV))
    return lrelu_act_masks(plan, RB_LEVEL, B, *d["meta"]["img"])


def _check_forward(tag, d, logits, loss):
    check_logits(tag, logits.cpu().double(), d["logits"].astype(np.float64))
    print(f"  loss {float(loss):.7f} vs {float(d['loss']):.7f}")
    assert abs(float(loss) - float(d["loss"])) <= 1e-5 * abs(float(d["loss"]))


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", ["unetr_same_k4", "unetr_resample_b2"])
def test_unetr_matches_fixture_and_kink_consistent_oracle(name, mth):
    d = _fixture(name)
    lit = _lit(d, mth)
    logits, loss = _step(lit, d)
    _check_forward(f"{name}/{mth}", d, logits, loss)
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    ref = {}
    U.ACT_MASKS = _engine_act_masks(lit, d)
    try:
        for dt in (torch.float64, torch.float32):
            ref[dt] = U.fwd_bwd(U.build(d["meta"], d["state"], dt), x, y, d["meta"])[2]
    finally:
        U.ACT_MASKS = None
    named = dict(lit.net.net.named_parameters())
    g64 = ref[torch.float64]
    rows = grad_errors({k: named[k].grad for k in g64}, g64, ref[torch.float32])
    check_grads_rows(rows, factor=16, top=6, width=56)
    unused = [k for k, p in named.items() if k not in ref[torch.float64]]
    assert unused and all("cross_attn" in k and named[k].grad is None for k in unused)


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
def test_unetr_registry_width_matches_fixture(mth):
    """216 tokens, 12 heads of 64, resampled (16, 48, 48) <-> 96^3.  Gradients against the
    stored head / tail / sum of the reference's fp32 run: the head and tail entries, the l2
    norm (against the stored fp32 norm and the fp64 run's) and the sum, which is bounded by
    numel x the entry bound and so is the weakest of the three.  The fp32 oracle's error is
    the one the fixture records per tensor (the reference's fp32 run against its own fp64
    run), max|g| the fp64 run's."""
    d = _fixture("unetr_registry_k13")
    lit = _lit(d, mth)
    logits, loss = _step(lit, d)
    _check_forward(f"unetr_registry_k13/{mth}", d, logits, loss)
    rows, bad = [], []
    for k, p in lit.named_parameters():
        if "grad64/" + k not in d:
            assert p.grad is None and "cross_attn" in k
            continue
        _s, l2, e32abs, gmax = (float(v) for v in d["grad64/" + k])
        g = p.grad.detach().cpu().double().reshape(-1)
        tol = max(1e-3, 16 * e32abs / gmax)
        if "grad/" + k in d:
            e = float((g - torch.from_numpy(d["grad/" + k]).double().reshape(-1)).abs().max())
        else:
            e = max(float((g[:64] - torch.from_numpy(d["gradhead/" + k]).double()).abs().max()),
                    float((g[-64:] - torch.from_numpy(d["gradtail/" + k]).double()).abs().max()))
        en = abs(float(g.norm()) - l2) / l2
        if "gradsum/" + k in d:  # the stored fp32 [sum, l2 norm] of a tensor too large to store
            s32, l32 = (float(v) for v in d["gradsum/" + k])
            en = max(en, abs(float(g.norm()) - l32) / l32)
            # entries within tol max|g| each: the sums differ by at most numel times that
            es = abs(float(g.sum()) - s32) / (g.numel() * gmax)
        else:
            es = 0.0
        rows.append((e / gmax, en, tol, k))
        if not (e / gmax <= tol and en <= tol and es <= tol):
            bad.append(f"{k}: entries {e / gmax:.2e} norm {en:.2e} sum {es:.2e} (bound {tol:.2e})")
    rows.sort(reverse=True)
    print("\n".join(f"  {k:56s} entries {a:.2e}  norm {b:.2e}  bound {t:.2e}"
                    for a, b, t, k in rows[:6]))
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------ plan behaviour --
def test_unetr_two_steps_are_bitwise_equal():
    d = _fixture("unetr_resample_b2")
    lit = _lit(d, "f16x3")

    def step():
        logits, loss = _step(lit, d)
        grads = {k: p.grad.clone() for k, p in lit.named_parameters() if p.grad is not None}
        return logits.clone(), {"loss": loss.clone(), **grads}
    assert_steps_bitwise(step)


def test_unetr_inference_equals_training_forward():
    d = _fixture("unetr_resample_b2")
    lit = _lit(d, "f16x3")
    x = torch.from_numpy(d["x"]).to(DEV)
    assert_no_grad_forward_equals_train(lit, x)


def test_unetr_registry_training_step():
    from innovative3D.config import variant
    lit = variant("UNETR")[1]().to(DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 1, 5, 64, 64, generator=g).to(DEV)
    y = torch.randint(0, 13, (1, 5, 64, 64), generator=g)
    y[torch.rand(1, 5, 64, 64, generator=g) < 0.02] = 255
    logged = {}
    lit.log = lambda k, v, **kw: logged.__setitem__(k, float(torch.as_tensor(v).detach()))
    loss = lit.training_step((x, y.to(DEV)), 0)
    loss.backward()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and math.isfinite(logged["train_loss"])
    for k, p in lit.named_parameters():
        if "cross_attn" in k:
            assert p.grad is None, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            assert float(p.grad.abs().max()) > 0, k


def test_op_wrappers_reject_mismatched_shapes():
    qkv = torch.zeros(2 * 8, 3 * 2 * 16, device=DEV)
    O, lse = E.vit_attn_fwd(qkv, 2, 2)
    for bad in (lambda: E.vit_attn_fwd(qkv, 3, 2),                    # 16 rows, batch 3
                lambda: E.vit_attn_fwd(qkv[:, :95], 2, 2),            # not 3 * heads * d wide
                lambda: E.vit_attn_bwd(qkv, O[:-1], O, lse, 2, 2),
                lambda: E.vit_attn_bwd(qkv, O, O, lse[:, :1], 2, 2),
                lambda: E.resize3d_fwd(qkv, (4, 4, 4)),
                lambda: E.resize3d_bwd(torch.zeros(1, 4, 4, 4, 3, device=DEV), (4, 4))):
        with pytest.raises(E.SpffError):
            bad()
