"""The per-voxel stage oracle (tests/_stage_oracle.py) checked on the CPU: the captured
gradients are the right tensors, the hooks do not change the step, and the comparator
flags a defect on one row of voxels that the parameter-gradient check cannot see."""
import functools

import numpy as np
import torch

from _stage_oracle import failing, stage_bar, stage_errors, stage_grads
from oracle import spff_oracle as O

K, CIN, BASE = 13, 5, 32
SHAPE = (2, 5, 24, 40)      # configuration A of tests/test_gpu_stagewise_bwd.py


@functools.lru_cache(maxsize=None)
def _case():
    """One small default net and batch, and its fp64 stage run (shared, left unchanged)."""
    from innovative3D.synthetic import synthetic_batch
    from innovative3D.weightgen import synth_state
    B, D, H, W = SHAPE
    cfg = O.SpffCfg(in_ch=CIN, num_classes=K, base=BASE)
    shapes = [(k, v) for k, v in O.param_shapes(cfg, D).items()]
    st = synth_state(shapes, seed=31, mask_jitter=0.25)
    x, y = synthetic_batch(B, CIN, D, H, W, num_classes=K, ignore_frac=0.03, seed=32)
    run = stage_grads(cfg, st, x.numpy(), y.numpy(), None, torch.float64, keep_inputs=True)
    return cfg, st, x, y, run


def test_captured_gradients_give_the_weight_gradients():
    """For every conv, fp64 conv3d_weight(conv input, captured gradient at its output) is the
    weight's .grad to 1e-12 of its max: the captured tensors are dy1 / dy2."""
    _cfg, _st, _x, _y, run = _case()
    assert len(run.conv_in) == 14
    for name, inp in run.conv_in.items():
        B, C, D, H, W = run.shape[name]
        dy = torch.from_numpy(run.grad[name]).view(B, D, H, W, C).permute(0, 4, 1, 2, 3)
        g = run.param_grads[run.conv_w[name]]
        gw = torch.nn.grad.conv3d_weight(inp, g.shape, dy.contiguous(), padding=(1, 1, 1))
        e = float((gw - g).abs().max()) / float(g.abs().max())
        assert e <= 1e-12, (name, e)


def test_hooks_are_transparent():
    """With no masks forced, the hooked step's logits, loss and parameter gradients equal a
    plain O.fwd_bwd bitwise, in fp64 and in fp32."""
    cfg, st, x, y, run64 = _case()
    for dt in (torch.float64, torch.float32):
        run = run64 if dt == torch.float64 else stage_grads(cfg, st, x.numpy(), y.numpy(), None, dt)
        P = O.params_from_state(st, dtype=dt)
        logits, loss, _ce, _dice = O.fwd_bwd(P, x.to(dt), y, cfg)
        assert float(loss) == run.loss
        lg = logits.permute(0, 2, 3, 4, 1).reshape(-1, K).double().numpy()
        assert np.array_equal(lg, run.logits)
        assert set(run.param_grads) == {k for k, v in P.items() if v.grad is not None}
        for k, g in run.param_grads.items():
            assert torch.equal(g, P[k].grad), k
    # the module-level functions are restored
    assert O.conv_in_lrelu.__module__ == O.__name__ and O._cat.__module__ == O.__name__


def test_stages_are_complete_and_skip_share_is_separate():
    """Every stage the GPU test reads is there; an encoder output's total gradient is its
    skip share plus the MaxPool backward of the pooled gradient (zero off the argmax)."""
    _cfg, _st, _x, _y, run = _case()
    for blk in ("enc1", "enc2", "enc3", "bott", "dec3", "dec2", "dec1"):
        for s in ("y1", "y2", "out"):
            assert f"{blk}.{s}" in run.grad
    for k in (1, 2, 3):
        assert f"pool{k}" in run.grad and f"dec{k}.up" in run.grad and f"dec{k}.skip" in run.grad
        tot, skip = run.grad[f"enc{k}.out"], run.grad[f"dec{k}.skip"]
        pooled = tot - skip
        B, C, D, H, W = run.shape[f"enc{k}.out"]
        # one entry per 2 x 2 window carries the pooled gradient
        win = np.abs(pooled).reshape(B, D, H // 2, 2, W // 2, 2, C) > 0
        assert win.sum(axis=(3, 5)).max() <= 1
        ref = run.grad[f"pool{k}"].reshape(B, D, H // 2, W // 2, C)
        got = pooled.reshape(B, D, H // 2, 2, W // 2, 2, C).sum(axis=(3, 5))
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_comparator_sees_one_row_the_parameter_check_cannot():
    """The gap the GPU test closes.  enc1's dy2 with 1e-3 of its max added on one W-row (the
    last H-row of one (b, d) slab): the comparator names exactly that stage above the bar,
    every other stage stays at 0 -- and the same defect summed into enc1.body.0.weight.grad
    stays below the 1e-3 of the tensor's scale that check_grads accepts.
    Measured over all ten (b, d) slabs the weight gradient moves by 0.86e-3 .. 1.005e-3 of its
    max (the scale check_grads uses is the same here: max sum_b |g_b| = max|g|), i.e. a defect
    50 x the per-voxel bar sits AT the parameter bar; the slab used, (0, D - 1), gives
    0.94e-3.  By linearity the smallest defect the per-voxel bar flags, 2e-5 of max, moves that
    weight gradient by 2e-5 of its max, 50 x under what check_grads accepts."""
    cfg, st, x, y, run = _case()
    ref64 = run.flat()
    # (the fp32 run on the fp64 run's LeakyReLU signs and pool argmaxes, as on the GPU)
    ref32 = stage_grads(cfg, st, x.numpy(), y.numpy(), run.masks, torch.float32).flat()
    B, D, H, W = SHAPE
    key = "grad:enc1.y2"
    g = ref64[key]
    delta = np.zeros_like(g).reshape(B, D, H, W, BASE)
    delta[0, D - 1, H - 1, :, :] = 1e-3 * np.abs(g).max()
    engine = dict(ref64)
    engine[key] = g + delta.reshape(g.shape)
    rows = stage_errors(engine, ref64, ref32)
    assert len(rows) == len(ref64)
    bad = failing(rows)
    assert [k for k, _a, _b in bad] == [key], bad
    for k, e_gpu, e_32 in rows:
        if k == key:
            assert abs(e_gpu - 1e-3) <= 1e-9 and e_gpu > stage_bar(e_32)
        else:
            assert e_gpu == 0.0, k
        assert 0.0 < e_32 < 1e-5, (k, e_32)      # the fp32 oracle's own per-voxel error
    # the same defect as check_grads sees it: through the weight gradient's sum over voxels
    name = "enc1.y2"
    gw = run.param_grads[run.conv_w[name]]
    dy = torch.from_numpy(delta).permute(0, 4, 1, 2, 3).contiguous()
    dgw = torch.nn.grad.conv3d_weight(run.conv_in[name], gw.shape, dy, padding=(1, 1, 1))
    e_param = float(dgw.abs().max()) / float(gw.abs().max())
    # check_grads' scale: max over the tensor of sum_b |per-sample gradient| (>= max|g|)
    dyf = torch.from_numpy(g).view(B, D, H, W, BASE).permute(0, 4, 1, 2, 3).contiguous()
    absb = sum(torch.nn.grad.conv3d_weight(run.conv_in[name][b:b + 1], gw.shape, dyf[b:b + 1],
                                           padding=(1, 1, 1)).abs() for b in range(B))
    assert float(absb.max()) >= float(gw.abs().max()) * (1 - 1e-12)
    e_param = float(dgw.abs().max()) / float(absb.max())
    print(f"one-row defect: per voxel 1.0e-03 of max, in {run.conv_w[name]}.grad {e_param:.2e}")
    assert e_param < 1e-3
