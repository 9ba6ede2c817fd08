"""CBAM spatial attention of the SPCT core on the device, op level: spff_spatial_attn_fwd /
spff_spatial_attn_bwd against fp64 torch on the host.

Bound, the rule tests/test_gpu_unetr.py uses for its ops: 16 x the error the same fp32
computation in torch on the CPU shows against fp64 for that case and output, floored at
1e-6 of max|ref|; both figures are printed.  The inputs carry a unique channel max per
voxel (one channel is lifted 0.25 above the rest), so the argmax index is compared exactly.

Shapes: the smallest volume, ragged tiles with a stencil wider than the plane, every
lanes-per-row path (C = 8, 24, 32, 64, 256; 24 has rows of unequal chunk counts), and
108 and 4100 tiles, which take two and three levels of the weight gradient's row
reduction."""
import pytest
import torch
import torch.nn.functional as F

from _compare import fp32_bound
from innovative3D import _engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 1, 1, 8), (2, 3, 5, 9, 8), (1, 2, 7, 7, 64), (1, 5, 24, 40, 32),
          (1, 2, 3, 5, 256), (2, 6, 33, 40, 24), (1, 4100, 1, 1, 8)]


def _case(shape):
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * C + D * H * W)
    x = torch.randn(B, D, H, W, C, generator=g)
    top = torch.randint(0, C, (B, D, H, W, 1), generator=g)
    x.scatter_(4, top, x.amax(dim=4, keepdim=True) + 0.25)
    w = torch.randn(1, 2, 3, 7, 7, generator=g) * 0.1
    dy = torch.randn(B, D, H, W, C, generator=g)
    return x, w, dy, top[..., 0]


def _torch_ref(x, w, dy, dt):
    """SpatialAttention3D.forward (mean, max, cat, conv, sigmoid, multiply) on channel-first
    views of the channel-last tensors -> y, attn, dx, dw."""
    a = x.to(dt).permute(0, 4, 1, 2, 3).requires_grad_(True)
    ww = w.to(dt).requires_grad_(True)
    m = torch.cat([a.mean(dim=1, keepdim=True), a.max(dim=1, keepdim=True)[0]], dim=1)
    attn = torch.sigmoid(F.conv3d(m, ww, padding=(1, 3, 3)))
    y = a * attn
    dx, dw = torch.autograd.grad(y, (a, ww), dy.to(dt).permute(0, 4, 1, 2, 3))
    cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous()
    return {"y": cl(y), "attn": attn.detach()[:, 0], "dx": cl(dx), "dw": dw}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spatial_attn_matches_fp64(shape):
    x, w, dy, top = _case(shape)
    ref, cpu32 = _torch_ref(x, w, dy, torch.float64), _torch_ref(x, w, dy, torch.float32)
    xd, wd = x.to(DEV), w.to(DEV)
    y, attn, amap, idx = E.spatial_attn_fwd(xd, wd)
    dx, dw = E.spatial_attn_bwd(dy.to(DEV), xd, wd, attn, amap, idx)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().long(), top)
    assert torch.equal(idx.cpu().long(), x.double().argmax(dim=4))
    assert torch.equal(amap[..., 1].cpu(), x.amax(dim=4))
    got = {"y": y, "attn": attn, "dx": dx, "dw": dw}
    bad = []
    for name in ("y", "attn", "dx", "dw"):
        bound, e32, ref_max = fp32_bound(ref[name], cpu32[name])
        err = float((got[name].cpu().double() - ref[name]).abs().max())
        print(f"[spatial_attn {shape}] {name}: err {err:.3e}  cpu-fp32 err {e32:.3e}  "
              f"bound {bound:.3e}  max|ref| {ref_max:.3e}")
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad


def test_spatial_attn_is_deterministic():
    x, w, dy, _ = _case((2, 6, 33, 40, 24))
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    runs = []
    for _ in range(2):
        y, attn, amap, idx = E.spatial_attn_fwd(xd, wd)
        runs.append((y, attn, amap, idx) + E.spatial_attn_bwd(dyd, xd, wd, attn, amap, idx))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_spatial_attn_lowest_index_takes_a_tie():
    """An exact tie of the channel max: the lowest channel index is stored and takes the max
    branch's gradient (torch.max's rule on the CPU, which the fp64 reference follows)."""
    x, w, dy, top = _case((1, 2, 5, 9, 32))
    x[..., 29] = x[..., 5] = x.amax(dim=4)
    xd, wd = x.to(DEV), w.to(DEV)
    _y, attn, amap, idx = E.spatial_attn_fwd(xd, wd)
    assert torch.equal(idx.cpu().long(), top.clamp(max=5))
    dx, _dw = E.spatial_attn_bwd(dy.to(DEV), xd, wd, attn, amap, idx)
    ref, cpu32 = _torch_ref(x, w, dy, torch.float64), _torch_ref(x, w, dy, torch.float32)
    bound, e32, _ = fp32_bound(ref["dx"], cpu32["dx"])
    err = float((dx.cpu().double() - ref["dx"]).abs().max())
    print(f"[spatial_attn tie] dx: err {err:.3e}  cpu-fp32 err {e32:.3e}  bound {bound:.3e}")
    assert err <= bound


# ---------------------------------------------------------------- whole net --
# The rules of tests/test_gpu_resunetpp.py: max|dlogit| <= 1e-3, at most 8 argmax flips, all
# at near-ties (top-2 margin below 2 x the error), loss within 1e-5 relative; every parameter
# gradient against the fp64 test oracle (tests/_spatial_oracle.py) run with the engine's own
# branch decisions -- LeakyReLU signs and pool argmaxes (_spff_checks.engine_branch_masks),
# the sa argmax indices and the gates' ReLU signs read through plan.saved -- within
# max(1e-3, 8 x the fp32 oracle's error), scaled by max|ref|.
import math  # noqa: E402


import _spatial_oracle as S  # noqa: E402
import innovative3D.helpers as Hh  # noqa: E402
import innovative3D.models as M  # noqa: E402
from _compare import (assert_no_grad_forward_equals_train, assert_steps_bitwise,  # noqa: E402
                      check_grads_rows, check_logits, grad_errors)
from _golden import cfg_of, load, state_of  # noqa: E402
from _spff_checks import engine_branch_masks, oracle_grads_st  # noqa: E402

FIXTURES = ("spa_full_b8", "spa_only_d1", "spa_ragged_hw", "gate_only_cin5", "spa_lit_k13")
LVL = {"enc1": 0, "enc2": 1, "enc3": 2, "bott": 3, "g1": 0, "g2": 1, "g3": 2}


def build_fixture_core(d, mth=None):
    """The engine-backed module of a fixture with its parameters loaded; -> (module, core)."""
    meta = d["meta"]
    fl = dict(use_se=meta["se"], use_specse=meta["specse"], use_spatial=meta["spatial"],
              use_skip_gate=meta["skip_gate"])
    if meta["lit"]:
        top = M.LitSPCT_EFiLM_FourierGate(num_classes=meta["K"], base=meta["base"], **fl)
        core = top.model
    else:
        core = M.UNet3D_SpectralCore(in_channels=meta["in_ch"], num_classes=meta["K"],
                                     base=meta["base"], ksd=3, **fl)
        if meta["efilm"] or meta["fgate"]:
            core = M.upgrade_spct_with_novel_blocks(core, use_efilm=meta["efilm"],
                                                    use_fouriergate=meta["fgate"])
        top = core
    for b in core._blocks():
        if isinstance(getattr(b, "fgate", None), M.FourierGate3D):
            b.fgate._ensure_mask(d["x"].shape[2], "cpu")
    core.load_state_dict({k: torch.from_numpy(v) for k, v in state_of(d).items()}, strict=True)
    if mth:
        core.math = mth
    return top.to(DEV), core


def engine_masks(core, d):
    """every branch decision of the engine's last forward, as the oracle's hooks take them"""
    meta, shape = d["meta"], d["x"].shape
    B, _, D, H, W = shape
    masks = engine_branch_masks(core, shape, state_of(d), cfg_of(meta))
    extra, plan = {}, core._plan
    if meta["spatial"]:
        for st in S.STAGES:
            extra[st + ".sa.idx"] = plan.saved(st + ".sa.idx").cpu().view(
                B, D, H >> LVL[st], W >> LVL[st]).long()
    if meta["skip_gate"]:
        for g in S.GATES:
            att = plan.saved(g + ".att").cpu()
            extra[g + ".att"] = (att.view(B, D, H >> LVL[g], W >> LVL[g], -1) > 0).permute(
                0, 4, 1, 2, 3).contiguous()
    return masks, extra


def train_step(core, d):
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    for p in core.parameters():
        p.grad = None
    logits = core(x)
    loss, _conf = Hh.ce_dice_with_confusion(logits, y, d["meta"]["K"], 255)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach()


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", FIXTURES)
def test_network_matches_reference(name, mth):
    d = load(name)
    meta = d["meta"]
    _top, core = build_fixture_core(d, mth)
    logits, loss = train_step(core, d)
    check_logits(f"{name}/{mth}", logits, d["logits"], max_flips=8)
    print(f"  loss {float(loss):.7f} vs {float(d['loss']):.7f}")
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    masks, extra = engine_masks(core, d)
    with S.as_oracle_forward(meta["spatial"], meta["skip_gate"]), S.forced_spatial(extra):
        g64, g32, nflip, _absb = oracle_grads_st(cfg_of(meta), state_of(d), d["x"], d["labels"],
                                                 masks)
    print(f"  LeakyReLU / pool knife-edge flips (engine vs fp64): {nflip}")
    named = {k: v for k, v in core.named_parameters(remove_duplicate=False)
             if not k.endswith("._mask")}
    assert set(named) == set(g64)
    check_grads_rows(grad_errors({k: named[k].grad for k in g64}, g64, g32), top=6, width=36)


@pytest.mark.parametrize("name", ["spa_full_b8", "spa_ragged_hw"])
def test_no_grad_forward_is_the_train_forward(name):
    d = load(name)
    _top, core = build_fixture_core(d)
    logits, _loss = train_step(core, d)  # a backward lies between that forward and the next
    lg = assert_no_grad_forward_equals_train(core, torch.from_numpy(d["x"]).to(DEV))
    assert torch.equal(lg, logits)


def test_forward_backward_is_deterministic():
    d = load("spa_full_b8")
    _top, core = build_fixture_core(d)

    def step():
        logits, _loss = train_step(core, d)
        return logits.clone(), {k: p.grad.clone() for k, p in core.named_parameters()}
    _logits, grads = assert_steps_bitwise(step)
    assert len(grads) >= 40


def test_lit_training_step_and_adam():
    d = load("spa_lit_k13")
    lit, core = build_fixture_core(d)
    lit.log = lambda *a, **k: None
    batch = (torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["labels"]).to(DEV))
    opt = torch.optim.Adam(lit.parameters(), lr=1e-3)
    loss = lit.training_step(batch, 0)
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    keys = [k for k, _ in core.named_parameters() if k.startswith(("sa.", "g1.", "g2.", "g3."))]
    assert len(keys) == 4 + 3 * 6
    before = {k: v.detach().clone() for k, v in core.named_parameters() if k in keys}
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    after = dict(core.named_parameters())
    for k in keys:
        assert not torch.equal(after[k].detach(), before[k]), k
