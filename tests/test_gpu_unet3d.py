"""3DUNet baseline variant (BASELINE config 3) on the HIP engine against the
fixtures the reference itself produced (tests/golden/fxu3d_*).  Marked gpu.

Checks, per fixture and conv arithmetic (f32, bf16x6): train-mode logits within
1e-3 of the reference PyTorch-CPU forward with identical argmax (near-ties
within 2 x max|dlogit| reported, not failed), the wrapper's weighted CE within
1e-5 relative, per_class_metrics_3d exactly, BatchNorm running statistics after
the step (1e-5 relative) and num_batches_tracked, eval-mode logits on the
updated statistics within 1e-3, and every parameter gradient against a
kink-consistent fp64 oracle within max(1e-3, 8 x the fp32 oracle's own error)
of max|g| (ReLU signs and max-pool argmaxes routed as the engine saw them:
an activation within fp32 rounding of 0 may legitimately take either side)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _compare import check_grads_rows, check_logits, grad_errors, kink_hooks, ncdhw, track_plan
from _golden import free_port, load, unet3d_fixture_names, unet3d_state_of
from oracle import unet3d_oracle as U
import innovative3D.models as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cfg_of(meta):
    return U.UNet3DCfg(num_classes=meta["K"], base=meta["base"], in_ch=meta["in_ch"],
                       target_depth=meta["target_depth"])


def build(d):
    meta = d["meta"]
    if meta.get("lit"):
        kw = {"class_weights": d["class_weights"].tolist()} if "class_weights" in d else {}
        m = M.LitCicek3DUNet_DepthAdapter_Published(num_classes=meta["K"], **kw)
    else:
        m = M.Cicek3DUNet(num_classes=meta["K"], base=meta["base"])
    st = unet3d_state_of(d)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    return m.to(DEV)


def engine_hooks(net, B, Dt, H, W):
    """ReLU sign patterns and pool argmaxes as the engine saw them (its saved
    block outputs), for the kink-consistent oracle."""
    plan = net._last_plan
    vols = {n: (Dt >> l, H >> l, W >> l) for n, l in
            zip(U.BLOCKS, (0, 1, 2, 3, 4, 3, 2, 1, 0))}
    masks, pidx = {}, {}
    for n in U.BLOCKS:
        D_, H_, W_ = vols[n]
        for s in ("a1", "out"):
            masks[f"{n}.{s}"] = ncdhw(plan.saved(f"{n}.{s}").cpu(), B, D_, H_, W_) > 0
    for l, n in enumerate(("enc1", "enc2", "enc3", "enc4")):
        D_, H_, W_ = vols[n]
        e = ncdhw(plan.saved(f"{n}.out").cpu(), B, D_, H_, W_)
        pidx[f"pool{l + 1}"] = F.max_pool3d(e, 2, return_indices=True)[1]
    return kink_hooks(masks, pidx)[0]


def oracle_grads(d, hooks, dtype):
    meta = d["meta"]
    pre = "backbone." if meta.get("lit") else ""
    P, Bf = U.params_from_state(unet3d_state_of(d), dtype=dtype, prefix=pre)
    x = torch.from_numpy(d["x"]).to(dtype)
    y = torch.from_numpy(d["labels"])
    cw = torch.from_numpy(d["class_weights"]).to(dtype) if "class_weights" in d else None
    lg = U.forward(P, Bf, x, cfg_of(meta), True, hooks)
    loss = U.weighted_ce(lg, y, 255, cw)
    loss.backward()
    return {k: v.grad.detach().double().numpy() for k, v in P.items()}


@pytest.mark.parametrize("mth", ["f32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("name", unet3d_fixture_names())
def test_unet3d_matches_reference(name, mth):
    d = load(name)
    meta = d["meta"]
    K = meta["K"]
    m = build(d)
    net = m.backbone if meta.get("lit") else m
    net.math = mth
    track_plan(net)
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    m.train()
    logits = m(x)
    if meta.get("lit"):
        loss = m._weighted_softmax_ce(logits, y, None)
        conf = m._last_conf
    else:
        from innovative3D import _engine as E
        loss, conf = M._WeightedCE.apply(logits, y, K, 255, None)
    loss.backward()
    torch.cuda.synchronize()
    lg = logits.detach().cpu().numpy()
    ref = d["logits"]
    _err, _nf, flips = check_logits(f"{name}/{mth}", lg, ref)
    print(f"  loss {float(loss):.7f} vs {float(d['loss']):.7f}")
    assert math.isclose(float(loss), float(d["loss"]), rel_tol=1e-5)
    met = M.metrics_from_confusion(conf.cpu().numpy(), K, int(y.numel()))
    if not flips.any():
        np.testing.assert_allclose(np.array(met[0]), d["met_dice"], rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(np.array(met[3:]), d["met_scalars"], rtol=1e-12, equal_nan=True)
    # BatchNorm running statistics and num_batches_tracked after the step
    sd = m.state_dict()
    for k in d:
        if k.startswith("bufafter/"):
            key = k[len("bufafter/"):]
            np.testing.assert_allclose(sd[key].cpu().numpy(), d[k], rtol=1e-5, atol=1e-6,
                                       err_msg=key)
        if k.startswith("nbt/"):
            assert int(sd[k[len("nbt/"):]]) == int(d[k])
    # gradients vs the kink-consistent fp64 oracle
    Bn, Dt = d["x"].shape[0], meta["target_depth"] or d["x"].shape[2]
    hooks = engine_hooks(net, Bn, Dt, d["x"].shape[3], d["x"].shape[4])
    g64 = oracle_grads(d, hooks, torch.float64)
    g32 = oracle_grads(d, hooks, torch.float32)
    pre = "backbone." if meta.get("lit") else ""
    named = dict(m.named_parameters())
    check_grads_rows(grad_errors({k: named[pre + k].grad for k in g64}, g64, g32), width=24)
    # eval mode: normalisation with the updated running statistics
    m.eval()
    with torch.no_grad():
        le = m(x).cpu().numpy()
    e_eval = float(np.abs(le - d["logits_eval"]).max())
    print(f"  eval-mode max|dlogit| = {e_eval:.3e}")
    assert e_eval <= 1e-3


def test_unet3d_config3_shape_step():
    """BASELINE config 3 shape: (4, 1, 5, 96, 96) -> depth adapter 16 -> back; one
    train step runs, logits finite, loss near ln(K) at init, every grad finite."""
    torch.manual_seed(0)
    m = M.LitCicek3DUNet_DepthAdapter_Published(num_classes=13).to(DEV)
    x = torch.randn(4, 1, 5, 96, 96, device=DEV)
    y = torch.randint(0, 13, (4, 5, 96, 96), device=DEV)
    logits = m(x)
    assert logits.shape == (4, 13, 5, 96, 96)
    loss = m._weighted_softmax_ce(logits, y, None)
    loss.backward()
    assert torch.isfinite(logits).all()
    assert abs(float(loss) - math.log(13)) < 1.0
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


# ---- data parallelism with synchronised BatchNorm ----
SB_SHAPE, SB_K = (4, 1, 5, 32, 32), 9


def _sb_model(seed=3):
    from innovative3D.weightgen import synth_state
    m = M.LitCicek3DUNet_DepthAdapter_Published(num_classes=SB_K)
    sd = m.state_dict()
    st = synth_state([(k, tuple(v.shape)) for k, v in sd.items()], seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return m.to(DEV).train()


def _sb_data():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(*SB_SHAPE, generator=g)
    G = torch.randn(SB_SHAPE[0], SB_K, *SB_SHAPE[2:], generator=g)  # d loss / d logits
    return x, G


def _sb_step(m, x, G):
    """forward (train mode) + a loss that is a plain sum over samples, so the batch's
    gradient is the SUM of the ranks' gradients with no loss normalisation in between"""
    for p in m.parameters():
        p.grad = None
    logits = m(x.to(DEV))
    (logits * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return logits.detach().cpu()


def _sb_worker(rank, world, port, out, sync):
    import os
    import pathlib
    import sys
    import torch.distributed as dist
    root = pathlib.Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root), str(root / "tests"), str(root / "spff-unet-spcct_amd")]
    from innovative3D.distributed import allreduce_gradients, sync_batchnorm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    m = _sb_model()
    if sync:
        sync_batchnorm(m)
    x, G = _sb_data()
    n = SB_SHAPE[0] // world
    lg = _sb_step(m, x[rank * n:(rank + 1) * n], G[rank * n:(rank + 1) * n])
    allreduce_gradients(list(m.parameters()))  # host-staged gloo: CPU copies
    bufs = {k: v.detach().cpu().numpy() for k, v in m.named_buffers() if "running" in k}
    np.savez(f"{out}.{rank}.npz", logits=lg.numpy(), **{"b_" + k: v for k, v in bufs.items()},
             **{"g_" + k: p.grad.cpu().numpy() for k, p in m.named_parameters()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mth", ["f32", "f16x3"])
def test_sync_batchnorm_world2_matches_single_batch(tmp_path, mth, monkeypatch):
    """(2 + 2) x 1 x 5 x 32^2 on two ranks with synchronised BatchNorm (host-staged gloo,
    both ranks on this GPU) against ONE process on the batch of 4: logits, running
    statistics and the all-reduced gradients.  Without SyncBN the ranks normalise with
    their own half-batch statistics, and the logits differ by O(1) (checked too)."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("SPFF_MATH", mth)
    m = _sb_model()
    x, G = _sb_data()
    ref = _sb_step(m, x, G).numpy()
    ref_g = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    ref_b = {k: v.detach().cpu().numpy() for k, v in m.named_buffers() if "running" in k}
    del m
    res = {}
    for sync in (True, False):
        out = str(tmp_path / f"sb{int(sync)}")
        mp.spawn(_sb_worker, args=(2, free_port(), out, sync), nprocs=2, join=True)
        parts = [np.load(f"{out}.{r}.npz") for r in range(2)]
        res[sync] = parts
    parts = res[True]
    lg = np.concatenate([p["logits"] for p in parts], axis=0)
    e = float(np.abs(lg - ref).max()) / float(np.abs(ref).max())
    e_nosync = float(np.abs(np.concatenate([p["logits"] for p in res[False]], 0) - ref).max()) \
        / float(np.abs(ref).max())
    worst_b = max(float(np.abs(parts[r]["b_" + k] - v).max() / max(np.abs(v).max(), 1e-30))
                  for k, v in ref_b.items() for r in range(2))
    rows = sorted(((float(np.abs(parts[0]["g_" + k] - v).max() / max(np.abs(v).max(), 1e-30)),
                    float(np.linalg.norm(parts[0]["g_" + k] - v) / max(np.linalg.norm(v), 1e-30)), k)
                   for k, v in ref_g.items()), reverse=True)
    worst_g = rows[0][0]
    worst_l2 = max(r[1] for r in rows)
    print(f"SyncBN world 2 {mth}: logits rel {e:.2e} (per-replica BN: {e_nosync:.2e}), running "
          f"stats rel {worst_b:.2e}, gradients max rel {worst_g:.2e}, rel L2 {worst_l2:.2e}")
    for mx, l2, k in rows[:4]:
        print(f"    {k:40s} max rel {mx:.2e}  rel L2 {l2:.2e}")
    assert e <= 1e-5, e
    assert e_nosync > 1e-2  # the test discriminates: per-replica statistics differ
    assert worst_b <= 1e-5, worst_b
    if mth == "f32":
        # the fp32 path's forward is bitwise the batch-of-4 one (same tiles and splits)
        assert worst_g <= 1e-4, worst_g
    else:
        # f16x3: the ranks' launches take their operand scales (and the small levels their
        # split-K partition) from their own half batch, so the forward differs in the last
        # bits (logits 3e-7) and a ReLU input on its knife edge can take the other side --
        # at the bottleneck a channel's BatchNorm spans 16 voxels, so one such flip moves
        # that channel's gamma / beta gradient by ~1e-3 of the tensor's max (measured);
        # the tensors as a whole stay within 1e-3 relative L2
        assert worst_l2 <= 1e-3, rows[:4]
    for k in ref_g:  # every rank holds the same reduced gradient
        np.testing.assert_array_equal(parts[0]["g_" + k], parts[1]["g_" + k])
