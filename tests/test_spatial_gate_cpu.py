"""Spatial attention and gated skips of the SPCT core, CPU side: the test oracle
(tests/_spatial_oracle.py) against the fixtures the reference wrote
(tests/golden/make_golden_spatial.py), the module tree and the plan's parameter table
against the fixtures' state dicts, the plan's refusals, and the unchanged default layout.
No GPU calls."""
import json
import math
import pathlib

import numpy as np
import pytest
import torch

import _spatial_oracle as S
import innovative3D.models as M
from _golden import cfg_of, load, state_of
from _kink import resolve_kinks
from innovative3D import _engine as E
from oracle import spff_oracle as O

NAMES = ("spa_full_b8", "spa_only_d1", "spa_ragged_hw", "gate_only_cin5", "spa_lit_k13")
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def flags_of(meta):
    return bool(meta["spatial"]), bool(meta["skip_gate"])


def grad_err(d, G):
    """worst gradient error of G against fixture d, relative to max|ref| per tensor (the rule
    of tests/test_oracle_golden.py: full tensors, or head / tail / L2 norm of the large ones)"""
    prefix = "model." if d["meta"].get("lit") else ""
    worst = 0.0
    for k in d["param_names"]:
        k = str(k)
        g = G[k[len(prefix):].replace("._mask", ".freq_mask")]
        if "grad/" + k in d:
            ref = d["grad/" + k]
            worst = max(worst, float(np.abs(g - ref).max()) / max(1e-6, float(np.abs(ref).max())))
        else:
            flat = g.reshape(-1)
            sc = max(1e-6, float(np.abs(d["gradhead/" + k]).max()))
            worst = max(worst, float(np.abs(flat[:64] - d["gradhead/" + k]).max()) / sc,
                        float(np.abs(flat[-64:] - d["gradtail/" + k]).max()) / sc)
            s_ = float(d["gradsum/" + k][1])
            worst = max(worst, abs(float(np.sqrt((flat ** 2).sum())) - s_) / max(s_, 1e-9))
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference(name):
    d = load(name)
    cfg, st = cfg_of(d["meta"]), state_of(d)
    x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    with S.as_oracle_forward(*flags_of(d["meta"])):
        P = O.params_from_state(st)
        logits, loss, ce, dice = O.fwd_bwd(P, x, y, cfg)
        ref = d["logits"]
        err = float(np.abs(logits.numpy() - ref).max())
        assert err <= 2e-5, err
        assert torch.equal(logits.argmax(1), torch.from_numpy(ref).argmax(1))
        assert math.isclose(float(ce), float(d["ce"]), rel_tol=1e-5)
        assert math.isclose(dice, float(d["dice_loss"]), rel_tol=0, abs_tol=1e-12)
        assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
        tol = 5e-4 if d["x"].shape[0] == 1 else 2e-3
        _, flips, e = resolve_kinks(st, x, y, cfg, lambda G: grad_err(d, G), tol)
    print(f"{name}: knife-edge flips {flips}, worst gradient error {e:.2e}")
    assert e <= tol and len(flips) <= 3, (flips, e)


def test_fixture_metas_record_the_reference_margins():
    for name in NAMES:
        m = load(name)["meta"]
        assert m["ref_flips32"] <= 2 and m["ref_err32"] < 2e-5, (name, m)
        assert len(m["sa_min_gap"]) == (4 if m["spatial"] else 0)
        assert all(g >= 1e-5 for g in m["sa_min_gap"]), (name, m)
        assert (GOLDEN / f"{name}.npz").stat().st_size < 1 << 20


def _plan_of(d, **kw):
    m = d["meta"]
    B, Cin, D, H, W = d["x"].shape
    return E.Plan(B, Cin, D, H, W, m["K"], base=m["base"], efilm=m["efilm"], fgate=m["fgate"],
                  se=m["se"], specse=m["specse"], spatial=m["spatial"], skip_gate=m["skip_gate"],
                  **kw)


def _module_of(meta):
    fl = dict(use_se=meta["se"], use_specse=meta["specse"], use_spatial=meta["spatial"],
              use_skip_gate=meta["skip_gate"])
    if meta["lit"]:
        return M.LitSPCT_EFiLM_FourierGate(num_classes=meta["K"], base=meta["base"], **fl)
    core = M.UNet3D_SpectralCore(in_channels=meta["in_ch"], num_classes=meta["K"],
                                 base=meta["base"], ksd=3, **fl)
    if meta["efilm"] or meta["fgate"]:
        core = M.upgrade_spct_with_novel_blocks(core, use_efilm=meta["efilm"],
                                                use_fouriergate=meta["fgate"])
    return core


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_and_plan_parameters_follow_the_reference(name):
    d = load(name)
    meta = d["meta"]
    ref = {k: tuple(v) for k, v in d["state_shapes"].items()}
    prefix = "model." if meta["lit"] else ""
    # the test oracle's table
    mine = S.param_shapes(cfg_of(meta), D=d["x"].shape[2], prefix=prefix,
                          spatial=meta["spatial"], skip_gate=meta["skip_gate"])
    assert list(mine) == list(ref) and all(tuple(mine[k]) == ref[k] for k in ref)
    # the module tree (the FourierGate masks appear at the first forward, as in the reference)
    top = _module_of(meta)
    for b in (top.model if meta["lit"] else top)._blocks():
        if isinstance(getattr(b, "fgate", None), M.FourierGate3D):
            b.fgate._ensure_mask(d["x"].shape[2], "cpu")
    sd = top.state_dict()
    assert list(sd) == list(ref), name
    assert all(tuple(sd[k].shape) == ref[k] for k in ref)
    if meta["skip_gate"]:
        assert float(sd[prefix + "g1.psi.bias"].abs().max()) == 0.0  # the reference's init
    # the plan's flat parameter table
    plan = _plan_of(d)
    order = [k[len(prefix):] for k in ref if not k.endswith("._mask")]
    assert [p[0] for p in plan.params] == order
    assert all(tuple(s) == ref[prefix + n] and k == int(np.prod(s)) for n, s, _o, k in plan.params)
    offs = [p[2] for p in plan.params]
    assert offs == sorted(offs) and plan.nfloats == offs[-1] + plan.params[-1][3]


def test_refusals():
    ok = dict(spatial=True, skip_gate=True)
    E.Plan(1, 1, 5, 16, 16, 4, base=8, **ok)
    for kw in (dict(spatial=True), dict(skip_gate=True)):
        with pytest.raises(E.SpffError, match=r"\(-1\).*unsharded"):   # SPFF_EINVAL
            E.Plan(1, 1, 5, 16, 16, 4, base=8, shard_world=2, shard_rank=0, **kw)
        with pytest.raises(E.SpffError, match=r"\(-1\).*unsharded"):
            E.Plan(2, 1, 5, 16, 16, 4, base=8, shard_world=2, shard_rank=1, shard_axis=1, **kw)
        with pytest.raises(E.SpffError, match=r"\(-1\).*lean"):
            E.Plan(1, 1, 5, 16, 16, 4, base=8, memory="lean", **kw)
    # auto resolves to the full layout when a flag is set, whatever the size
    big = dict(batch=1, in_ch=5, depth=512, height=512, width=512, num_classes=13)
    assert E.Plan(**big).layout == "lean"
    p = E.Plan(**big, spatial=True)
    assert p.layout == "full" and p.ws_bytes > E.Plan(**big, memory="full").ws_bytes
    # 18 -> 9 -> 4: the up-conv gives 8 against the skip's 9; the reference's gate fails there
    with pytest.raises(E.SpffError, match=r"\(-3\).*multiples of 8"):  # SPFF_ESHAPE
        E.Plan(1, 5, 2, 18, 20, 3, base=8, skip_gate=True)
    E.Plan(1, 5, 2, 18, 20, 3, base=8, spatial=True)  # spatial alone keeps ragged H, W


def test_python_wrappers_raise_before_a_device_call(monkeypatch):
    """sharded / lean / ragged-with-gate modules refuse in _engine_plan, before any plan or
    device call (the input here is a host tensor that never reaches the engine)"""
    monkeypatch.setattr(E, "get_plan", lambda **kw: pytest.fail("a plan was requested"))
    x = torch.zeros(1, 1, 5, 16, 16)
    core = M.UNet3D_SpectralCore(num_classes=4, base=8, use_spatial=True)
    core.shard = (2, 0)
    with pytest.raises(E.SpffError, match="unsharded"):
        core._engine_plan(x, "train")
    core = M.UNet3D_SpectralCore(num_classes=4, base=8, use_skip_gate=True)
    core.memory = "lean"
    with pytest.raises(E.SpffError, match="lean"):
        core._engine_plan(x, "train")
    core = M.UNet3D_SpectralCore(num_classes=4, base=8, use_skip_gate=True)
    with pytest.raises(E.SpffError, match="multiples of 8"):
        core._engine_plan(torch.zeros(1, 1, 2, 18, 20), "train")


def test_flags_off_keep_the_pinned_layout():
    import sys
    sys.path.insert(0, str(GOLDEN))
    import make_golden_plan_layouts as G
    record = json.loads((GOLDEN / "plan_layouts.json").read_text())
    n = 0
    for cid, cls, kw in G.CASES:
        if cls != "Plan":
            continue
        assert G.layout(E, cls, {**kw, "spatial": False, "skip_gate": False}) == record[cid], cid
        n += 1
    assert n >= 4
    # and a flag does move it
    a = G.layout(E, "Plan", G.CASES[0][2])
    b = G.layout(E, "Plan", {**G.CASES[0][2], "spatial": True})
    assert b["nfloats"] == a["nfloats"] + 4 * 294 and b["ws_bytes"] > a["ws_bytes"]


def test_registry_factory_takes_the_flags():
    from innovative3D.config import VARIANTS
    lit = dict((n, b) for n, b, *_ in VARIANTS)["SPFF-UNet"](use_spatial=True, use_skip_gate=True)
    core = lit.model
    assert all(isinstance(m, M.SpatialAttention3D) for m in core.sa)
    assert tuple(core.g3.W_x.weight.shape) == (64, 128, 1, 1, 1)
    assert tuple(core.g1.psi.weight.shape) == (1, 16, 1, 1, 1)
    for cls in (M.LitSPCT_EnergyFiLM, M.LitSPCT_FourierGate, M.LitSPCT_ControlUNet):
        m = cls(num_classes=3, base=8, use_spatial=True, use_skip_gate=True).model
        assert isinstance(m.sa[3], M.SpatialAttention3D) and m.g2 is not None
    assert M.build_spct_energyfilm_fourier(num_classes=3, base=8, use_spatial=True).g1 is None
