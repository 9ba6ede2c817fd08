"""UNETR variant: the registry entry, the engine mirror's module tree and flat layout, the
CPU oracle (tests/_unetr_oracle.py) against the fixtures the reference's LitUNETR_Published
produced around it (tests/golden/make_golden_unetr.py, unetr_*.npz), the resample
restatement, the argument checks and the learning-rate schedule.  CPU-only.

PARITY UNPINNED: the fixtures pin the reference's pad / resample / crop / loss / gradient
flow; the MONAI body inside them is the oracle's own restatement."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _unetr_oracle as U
from _golden import load, synth_state_of

NET_FIXTURES = ["unetr_same_k4", "unetr_resample_b2", "unetr_registry_k13"]


def test_registry_has_unetr(monkeypatch):
    from innovative3D import config as C
    name, factory, _dm, ckpt = C.variant("UNETR")
    assert name == "UNETR" and ckpt.name == "UNETR"
    names = [v[0] for v in C.VARIANTS]
    assert names[names.index("UNETR") + 1] == "3DUNet"
    assert len(names) == 10  # the reference's whole registry
    monkeypatch.setenv("INNOVATIVE3D_VARIANT", "UNETR")
    assert [v[0] for v in C.selected_variants()] == ["UNETR"]


def test_factory_builds_reference_hparams():
    from innovative3D import config as C
    import innovative3D.models as M
    lit = C.variant("UNETR")[1]()
    assert type(lit) is M.LitUNETR_Published
    ref = load("unetr_registry_k13")["meta"]["hparams"]
    got = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(lit.hparams).items()}
    assert got == ref
    assert "use_cosine_lr" not in got  # not a constructor argument: build_class drops it
    opt = lit.configure_optimizers()
    assert isinstance(opt, torch.optim.AdamW)
    assert opt.defaults["lr"] == 1e-4 and opt.defaults["weight_decay"] == 1e-2
    # the loss, schedule and optimiser are LitSwinUNETR_Published's own, shared
    for fn in ("_loss", "on_train_batch_start", "on_train_batch_end", "configure_optimizers"):
        assert getattr(M.LitUNETR_Published, fn) is getattr(M.LitSwinUNETR_Published, fn)


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_state_dict_and_flat_layout(name):
    import innovative3D.models as M
    from innovative3D import _engine as E
    d = load(name)
    m = d["meta"]
    lit = M.LitUNETR_Published(num_classes=m["K"], img_size=tuple(m["img"]),
                               feature_size=m["feature_size"], hidden_size=m["hidden"],
                               mlp_dim=m["mlp_dim"], num_heads=m["heads"], ignore_index=255,
                               include_bg_in_dice=False)
    sd = lit.state_dict()
    assert list(sd.keys()) == [str(k) for k in d["state_keys"]]
    assert {k: list(v.shape) for k, v in sd.items()} == d["state_shapes"]
    # a reference checkpoint loads strictly, the unused cross-attention holders included
    lit.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_of(d).items()}, strict=True)
    unused = [str(k) for k in d["unused_params"]]
    assert unused and all("cross_attn" in k for k in unused)
    try:
        E.lib()
    except E.SpffError:
        pytest.skip("libspff_hip.so is not built")
    B, _c, D, H, W = d["x"].shape
    pad = [-(-v // 16) * 16 for v in (D, H, W)]
    plan = E.UNETRPlan(B, 1, *pad, m["K"], img=tuple(m["img"]), feature_size=m["feature_size"],
                       hidden=m["hidden"], mlp_dim=m["mlp_dim"], heads=m["heads"])
    used = [k[len("net.net."):] for k in d["param_names"] if str(k) not in unused]
    assert [p[0] for p in plan.params] == used
    for pname, shape, _off, n in plan.params:
        assert list(shape) == d["state_shapes"]["net.net." + pname] and n == int(np.prod(shape))
    offs = [p[2] for p in plan.params]
    assert offs == sorted(offs) and plan.nfloats == offs[-1] + plan.params[-1][3]


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_oracle_reproduces_fixture(name):
    """The fp64 oracle against the reference's fp32 run.  Logits: 4 x the reference's own
    fp32-vs-fp64 error recorded in the fixture (floor 2e-5, the other variants' bar); loss
    1e-5 relative; every gradient's sum and l2 norm within 1e-6 of the reference's own fp64
    run; the stored fp32 gradient entries within 2 x the reference's own fp32 gradient error
    for that tensor."""
    d = load(name)
    meta = d["meta"]
    torch.set_num_threads(8)
    net = U.build(meta, synth_state_of(d))
    logits, loss, grads = U.fwd_bwd(net, torch.from_numpy(d["x"]), torch.from_numpy(d["labels"]),
                                    meta)
    ref = d["logits"]
    assert tuple(logits.shape) == ref.shape
    err = float(np.abs(logits.numpy() - ref).max())
    bound = max(2e-5, 4 * float(d["ref_err32"]))
    print(f"{name}: max|dlogit| = {err:.3e}  bound {bound:.3e} "
          f"(reference fp32 vs fp64: {float(d['ref_err32']):.3e})")
    assert err <= bound
    top2 = logits.topk(2, dim=1).values
    ties = (top2[:, 0] - top2[:, 1]) < 2 * max(err, 1e-12)
    assert not ((logits.argmax(1) != torch.from_numpy(ref).argmax(1)) & ~ties).any()
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    unused = {str(k) for k in d["unused_params"]}
    for k in d["param_names"]:
        k = str(k)
        short = k[len("net.net."):]
        if k in unused:
            assert short not in grads
            continue
        g = grads[short].numpy()
        s64 = d["grad64/" + k]
        # the fixture's fp32 entries: off the fp64 oracle by the reference's own fp32 error
        # (its fp32 run against its fp64 run, recorded per tensor), with a 2 x margin
        tol = 2 * float(s64[2]) + 1e-7 * float(s64[1])
        if "grad/" + k in d:
            assert float(np.abs(g - d["grad/" + k]).max()) <= tol, k
        else:
            flat = g.reshape(-1)
            assert float(np.abs(flat[:64] - d["gradhead/" + k]).max()) <= tol, k
            assert float(np.abs(flat[-64:] - d["gradtail/" + k]).max()) <= tol, k
        # fp64 against the reference's own fp64 run: no fp32 rounding, no knife edge
        flat = g.reshape(-1)
        assert math.isclose(float(np.sqrt((flat ** 2).sum())), float(s64[1]), rel_tol=1e-6,
                            abs_tol=1e-12), k
        assert math.isclose(float(flat.sum()), float(s64[0]), rel_tol=1e-6,
                            abs_tol=1e-6 * float(s64[1])), k


def test_oracle_loss_matches_reference():
    z = np.load(load.__globals__["GOLDEN"] / "unetr_loss_small.npz")
    for c in [str(c) for c in z["cases"]]:
        t = torch.from_numpy(z[f"{c}/logits"]).double().requires_grad_(True)
        loss, _dice, _ce = U.lit_loss(t, torch.from_numpy(z[f"{c}/labels"]))
        loss.backward()
        assert math.isclose(float(loss.detach()), float(z[f"{c}/loss"]), rel_tol=1e-6), c
        ref = z[f"{c}/dlogits"]
        assert float(np.abs(t.grad.numpy() - ref).max()) <= 1e-6 * float(np.abs(ref).max()), c
    # case b holds a sample without foreground
    yb = z["b/labels"][1]
    assert not ((yb > 0) & (yb != 255)).any()


@pytest.mark.parametrize("src,dst,C", [((16, 80, 48), (48, 48, 48), 5),
                                       ((48, 48, 48), (16, 80, 48), 5),
                                       ((96, 96, 96), (16, 96, 64), 13)])
def test_resample_restatement_equals_interpolate(src, dst, C):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, C, *src, generator=g, dtype=torch.float64)
    dy = torch.randn(1, C, *dst, generator=g, dtype=torch.float64)
    out = []
    for fn in (lambda t: F.interpolate(t, size=dst, mode="trilinear", align_corners=False),
               lambda t: U.resize3d(t, dst)):
        a = x.clone().requires_grad_(True)
        y = fn(a)
        y.backward(dy)
        out.append((y.detach(), a.grad))
    assert float((out[0][0] - out[1][0]).abs().max()) <= 1e-12 * float(out[0][0].abs().max())
    assert float((out[0][1] - out[1][1]).abs().max()) <= 1e-12 * float(out[0][1].abs().max())


def test_argument_checks_return_einval():
    import ctypes
    from innovative3D import _engine as E
    L = E.lib()
    ok = dict(batch=1, in_ch=1, depth=32, height=32, width=32, num_classes=4, img=(32, 32, 32),
              feature_size=8, hidden=128, mlp_dim=256, heads=2)
    E.UNETRPlan(**ok)
    for bad, word in ((dict(img=(40, 32, 32)), "img must be multiples"),
                      (dict(hidden=130, heads=4), "multiple of heads"),
                      (dict(hidden=256, heads=2), "head width"),      # hd 128
                      (dict(hidden=96, heads=4), "head width"),       # hd 24
                      (dict(img=(128, 128, 160)), "512 tokens"),      # 640 tokens
                      (dict(depth=40), "multiples of 16"),
                      (dict(in_ch=2), "in_ch")):
        with pytest.raises(E.SpffError, match=word) as ei:
            E.UNETRPlan(**{**ok, **bad})
        assert "(-1)" in str(ei.value)  # SPFF_EINVAL
    # the exported op validates its geometry before it touches a pointer or the device
    for B, n, C, nh, word in ((1, 8, 130, 4, "multiple of heads"), (1, 8, 96, 4, "head width"),
                              (1, 600, 128, 2, "512 tokens"), (0, 8, 128, 2, "positive")):
        rc = L.spff_vit_attn_fwd(None, B, n, C, nh, None, None, None)
        assert rc == -1 and word in L.spff_last_error().decode()
        rc = L.spff_vit_attn_bwd(None, None, None, None, B, n, C, nh, None, None, None)
        assert rc == -1 and word in L.spff_last_error().decode()
    assert L.spff_resize3d_fwd(None, None, 1, 0, 4, 4, 4, 4, 4, 4, None) == -1
    assert L.spff_resize3d_bwd(None, None, 1, 3, 4, 4, 4, 0, 4, 4, None) == -1
    assert ctypes.sizeof(E.spff_unetr_cfg) == 20 * 4


def test_warmup_cosine_learning_rate():
    import innovative3D.models as M
    lit = M.LitUNETR_Published(num_classes=4, img_size=(32, 32, 32), feature_size=8,
                               hidden_size=128, mlp_dim=256, num_heads=2, lr=1e-4,
                               warmup_epochs=5)
    lit._total_train_iters = 100  # no trainer: one batch per epoch -> 5 warm-up iterations
    for t in (0, 1, 4, 5, 6, 52, 99, 100):
        lit._iters_done = t
        got = lit.on_train_batch_start(None, 0)
        assert math.isclose(got, U.lr_at(t, 1e-4, 5, 100), rel_tol=1e-12), t
    lit._iters_done = 0
    assert math.isclose(lit.on_train_batch_start(None, 0), 2e-5, rel_tol=1e-12)
    lit._iters_done = 5
    assert math.isclose(lit.on_train_batch_start(None, 0), 1e-4, rel_tol=1e-12)
    lit._iters_done = 100
    assert abs(lit.on_train_batch_start(None, 0)) < 1e-20
