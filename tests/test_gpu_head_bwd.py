"""The head's backward folded into the last decoder block's passes (csrc/norm.hip
k_head_tail_bwd: the head's weight / bias gradient and dec1's six tail sums in one pass over
(y2, dlogits); k_in_bwd_apply_head: dec1's IN-backward apply forming the head's input
gradient from the dlogits rows) against the four passes it replaces (head_wgrad, head_dgrad,
the RED_BWD_TAIL6 slab_reduce, k_in_bwd_apply on a stored dout; debug key 4 = 0).

The fold needs the streaming head (base 32 or 64, K <= 32), which the base-16 parity tests
never reach.  dout is formed by the same fmaf chain either way, so the two paths sum the
same terms in another order: the logits are bitwise equal (the forward is untouched) and
every parameter gradient is within 1e-4 of its tensor's max |g| (the bound of
test_gpu_parity.py::test_fused_in_backward_sums for the same kind of change; observed
worst values are in profiles/head_fold/README.md).  The folded path is deterministic
(two runs bitwise equal) and replays bitwise from a captured HIP graph.  Marked gpu."""
import pytest
import torch

from _spff_checks import synth_core
import innovative3D.helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _core(K, base, D, mth, seed):
    core = synth_core(K, base, 5, D, seed)[0].to(DEV)
    core.math = mth
    return core


def _step(core, x, y, K, fold):
    for p in core.parameters():
        p.grad = None
    lg = core(x)
    core._plan.debug_set(4, fold)
    loss, _conf = Hh.ce_dice_with_confusion(lg, y, K, 255)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in core.named_parameters() if p.grad is not None}
    return lg.detach().clone(), grads


# (B, D, H, W), K, base, math:
#   (2, 8, 32, 48)    several slabs, several workgroups per slab, both arithmetics
#   (1, 5, 24, 40)    H W = 960 is no multiple of the 256-row tile, D odd: a ragged last tile
#   (1, 4, 16, 16)    K = 20: the K <= 32 instantiations; base 64: the C = 64 ones
#   (1, 4, 360, 368)  more than one 256-row tile per workgroup (the tile loop of both kernels,
#                     taken from 2^19 voxels up) with a ragged last one (H W = 517.5 x 256)
CASES = [((2, 8, 32, 48), 13, 32, "f16x3"), ((2, 8, 32, 48), 13, 32, "f32"),
         ((1, 5, 24, 40), 13, 32, "f16x3"), ((1, 4, 16, 16), 20, 32, "f16x3"),
         ((1, 4, 16, 16), 13, 64, "f16x3"), ((1, 4, 360, 368), 13, 32, "f16x3")]


@pytest.mark.parametrize("shape,K,base,mth", CASES)
def test_head_fold_matches_four_pass(shape, K, base, mth):
    from innovative3D.synthetic import synthetic_batch
    B, D, H, W = shape
    core = _core(K, base, D, mth, seed=13)
    x, y = synthetic_batch(B, 5, D, H, W, num_classes=K, ignore_frac=0.02, seed=14)
    x, y = x.to(DEV), y.to(DEV)
    assert int((y == 255).sum()) > 0  # ignored voxels: all-zero dlogits rows
    try:
        lg1, g1 = _step(core, x, y, K, 1)
        lg0, g0 = _step(core, x, y, K, 0)
        lg2, g2 = _step(core, x, y, K, 1)
    finally:
        core._plan.debug_set(4, 1)
    assert torch.equal(lg1, lg0) and torch.equal(lg1, lg2)
    assert g1.keys() == g0.keys() == g2.keys() and len(g1) > 20
    assert "out.weight" in g1 and "out.bias" in g1
    worst = max((float((g1[k] - g0[k]).abs().max() / g0[k].abs().max().clamp_min(1e-30)), k)
                for k in g0)
    print(f"head fold {shape} K {K} base {base} {mth}: worst gradient difference "
          f"{worst[0]:.2e} of max|g| ({worst[1]})")
    assert worst[0] <= 1e-4, worst
    # the key selects another code path (another summation order of the head's gradient):
    # a silent fall-back to the four passes would compare a path with itself
    assert any(not torch.equal(g1[k], g0[k]) for k in g0)
    for k in g1:  # determinism: fixed summation order, no atomics
        assert torch.equal(g1[k], g2[k]), k


def test_head_fold_graph_replay_equals_eager():
    """The folded step captured into a HIP graph (the shape of tests/test_gpu_graph.py, at
    base 32): loss and every gradient of a replay bitwise equal to the eager step, also
    after new inputs were copied into the captured buffers."""
    from innovative3D.distributed import DataParallelSPFF
    from innovative3D.synthetic import synthetic_batch
    K, D = 13, 16
    core = _core(K, 32, D, "f16x3", seed=11)
    runner = DataParallelSPFF(core, K, 255)
    x1, y1 = synthetic_batch(2, 5, D, 32, 48, num_classes=K, ignore_frac=0.02, seed=1)
    x2, y2 = synthetic_batch(2, 5, D, 32, 48, num_classes=K, ignore_frac=0.02, seed=2)
    x, y = x1.to(DEV), y1.to(DEV)

    def grads():
        return {k: p.grad.detach().clone() for k, p in core.named_parameters() if p.grad is not None}

    def eager(xx, yy):
        x.copy_(xx)
        y.copy_(yy)
        loss, _conf = runner.step(x, y)
        torch.cuda.synchronize()
        return float(loss), grads()

    ref1 = eager(x1, y1)
    ref2 = eager(x2, y2)
    x.copy_(x1)
    y.copy_(y1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runner.step(x, y)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gl, _gc = runner.step(x, y)
    for xx, yy, ref in ((x1, y1, ref1), (x2, y2, ref2), (x1, y1, ref1)):
        x.copy_(xx)
        y.copy_(yy)
        g.replay()
        torch.cuda.synchronize()
        assert float(gl) == ref[0]
        got = grads()
        assert got.keys() == ref[1].keys()
        for k in ref[1]:
            assert torch.equal(got[k], ref[1][k]), k
