"""Every stage of the engine's backward, per voxel, against the fp64 oracle.  Marked gpu.

check_grads (tests/_spff_checks.py) sees the backward only through parameter gradients,
each a sum over all voxels: a pass that is wrong on one row of a ragged tile, on the last
chunk of a split reduction or on one (b, d) slab stays far below its 1e-3
(tests/test_stage_oracle_cpu.py measures one such case).  Here the backward is stopped
after each block in turn (debug key 0) and the scratch it leaves -- the gradients at y2 and
y1, the block's input gradient, the skip's share, the gradient the up-conv handed down --
is compared voxel by voxel with the oracle's gradient at the same tensor
(tests/_stage_oracle.py), run with the engine's own LeakyReLU signs and pool argmaxes.
The forward stages the plan keeps are compared in the same run.

Bar, every comparison: max|a - g64| / max|g64| <= max(8 x e_32, 2e-5), e_32 the fp32
oracle's own error at that stage against fp64 (same forced branches), 8 the factor of
check_grads, 2e-5 of max what test_conv3d_fwd_dgrad_wgrad accepts of one fp32-MFMA conv.
f32, bf16x6 and f16x3 are held to the same bar.

Out of scope: use_spatial / use_skip_gate plans (ds lives in grad.dy2 and sa_bwd_step runs
first) and sharded plans.
"""
import pytest
import torch

from _golden import cfg_of, load, state_of
from _spff_checks import engine_branch_masks, load_core, synth_core
from _stage_oracle import failing, format_rows, stage_errors, stage_grads
from oracle import spff_oracle as O
import innovative3D.helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda"

# what each configuration is there for
CASES = {
    # ragged conv tiles; odd D (no Nyquist bin); HW = 960: slab_reduce in 2 splits with a
    # ragged second chunk at C = 32; level 3 is 3 x 5; the folded streaming head
    "A-f32": dict(base=32, shape=(2, 5, 24, 40), mth="f32"),
    "A-bf16x6": dict(base=32, shape=(2, 5, 24, 40), mth="bf16x6"),
    "A-f16x3": dict(base=32, shape=(2, 5, 24, 40), mth="f16x3"),
    # Cout < 32 convs; the non-streaming head (head_wgrad + head_dgrad); even D
    "B-f16x3": dict(base=16, shape=(2, 8, 32, 48), mth="f16x3"),
    # C x D >= SPFF_GSPLIT_MIN at every level: the k_gfs_* / k_gbs_* channel-split gate
    # kernels, at even and odd D
    "C256-f16x3": dict(base=32, shape=(1, 256, 8, 8), mth="f16x3"),
    "C257-f16x3": dict(base=32, shape=(1, 257, 8, 8), mth="f16x3"),
    # no tail: the RED_BWD_IN path of bwd_block
    "D-f32": dict(fixture="fxabl_PlainCore_UNet", mth="f32"),
    # the _cat resize and resize_hw_bwd
    "E-f32": dict(fixture="fx4_ragged_hw", mth="f32"),
    # the lean layout: only the views its backward does not reuse within a block
    "F-lean-f16x3": dict(base=32, shape=(2, 5, 24, 40), mth="f16x3", memory="lean"),
}
IN_CH, K_SYNTH = 5, 13
DEC = {1: "dec1", 2: "dec2", 3: "dec3"}            # stop k -> the block that ran last
ENC = {4: ("bott", "pool3"), 5: ("enc3", "pool2"), 6: ("enc2", "pool1")}


def _build(case):
    """(core on the device, cfg, state, x, labels) of a configuration"""
    if "fixture" in case:
        d = load(case["fixture"])
        core, cfg, st = load_core(d), cfg_of(d["meta"]), state_of(d)
        x, y = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"])
    else:
        from innovative3D.synthetic import synthetic_batch
        B, D, H, W = case["shape"]
        core, st = synth_core(K_SYNTH, case["base"], IN_CH, D, 31, 0.25)
        core = core.to(DEV)
        cfg = O.SpffCfg(in_ch=IN_CH, num_classes=K_SYNTH, base=case["base"])
        x, y = synthetic_batch(B, IN_CH, D, H, W, num_classes=K_SYNTH, ignore_frac=0.03, seed=32)
    core.math = case["mth"]
    if "memory" in case:
        core.memory = case["memory"]
    return core, cfg, st, x, y


@pytest.mark.parametrize("name", list(CASES))
def test_stagewise_backward(name):
    case = CASES[name]
    lean = case.get("memory") == "lean"
    core, cfg, st, x, y = _build(case)
    K = cfg.num_classes
    xd, yd = x.to(DEV), y.to(DEV)
    core(xd)                      # the training plan exists from the first forward on
    plan = core._plan
    engine = {}
    first = []

    def step(stop=-1, pool_fold=1, head_fold=1):
        """one forward + loss + backward, stopped after ``stop`` blocks; the forward is
        deterministic: its logits are bitwise those of the first step"""
        for p in core.parameters():
            p.grad = None
        logits = core(xd)
        plan.debug_set(0, stop)
        plan.debug_set(2, pool_fold)
        plan.debug_set(4, head_fold)
        loss, _conf = Hh.ce_dice_with_confusion(logits, yd, K, 255)
        loss.backward()
        torch.cuda.synchronize()
        if not first:
            first.append(logits.detach().clone())
        assert torch.equal(logits.detach(), first[0]), f"forward not repeatable (stop {stop})"

    def read(key, view, stage):
        """scratch view -> engine[key]: the flat prefix [V_l][C_l] of a level-0 view"""
        B_, C_, D_, H_, W_ = ref64.shape[stage]
        n = B_ * D_ * H_ * W_
        t = plan.saved(view).reshape(-1)
        assert t.numel() >= n * C_, (view, stage)
        engine[key] = t[:n * C_].view(n, C_).double().cpu().numpy()

    try:
        if not lean:
            plan.debug_set(1, 1)  # keep the GEMM-applied block outputs for the forward stages
        step(pool_fold=0)         # the whole backward, encoder output gradients materialised
        masks = engine_branch_masks(core, tuple(x.shape), st, cfg)
        ref64 = stage_grads(cfg, st, x.numpy(), y.numpy(), masks, torch.float64)
        ref32 = stage_grads(cfg, st, x.numpy(), y.numpy(), masks, torch.float32)
        # ---- forward stages of that run
        fwd = [f"{b}.{s}" for b in ("enc1", "enc2", "enc3", "bott", "dec3", "dec2", "dec1")
               for s in (("y1", "y2") if lean else ("y1", "y2", "out"))] + ["pool1", "pool2", "pool3"]
        for k in fwd:
            engine[k] = plan.saved(k).double().cpu().numpy()
        if not lean:              # (lean: the up-conv outputs live in backward scratch)
            for u in (1, 2, 3):
                engine[f"dec{u}.up"] = plan.saved(f"up{u}").double().cpu().numpy()
        # ---- after the whole backward, k_maxpool_bwd_add pass: enc1, and the totals
        read("grad:enc1.y2@pool-pass", "grad.dy2", "enc1.y2")
        read("grad:enc1.y1@pool-pass", "grad.da1", "enc1.y1")
        for lvl in range(3):
            read(f"grad:enc{lvl + 1}.out@pool-pass", f"grad.dskip{lvl}", f"enc{lvl + 1}.out")
        # ---- after the whole backward, PoolAdd fold (the default): enc1 again
        step()
        read("grad:enc1.y2", "grad.dy2", "enc1.y2")
        read("grad:enc1.y1", "grad.da1", "enc1.y1")
        # ---- stopped after each decoder block
        for stop, blk in DEC.items():
            for head_fold in ((1, 0) if stop == 1 and not lean else (1,)):
                step(stop=stop, head_fold=head_fold)
                tag = "" if head_fold else "@head-passes"
                # lean: lean_dec_input rebuilds the block's input in grad.out and (dec1, dec2:
                # the previous decoder's output) in grad.dy2 before the first conv's gradients
                if not lean:
                    read(f"grad:{blk}.y2{tag}", "grad.dy2", f"{blk}.y2")
                    # dec1's output gradient exists only where the head's input gradient
                    # is a pass of its own; dec2's and dec3's came through upconv_dgrad
                    if stop > 1 or not head_fold:
                        read(f"grad:{blk}.out{tag}", "grad.out", f"{blk}.out")
                read(f"grad:{blk}.y1{tag}", "grad.da1", f"{blk}.y1")
                read(f"grad:{blk}.up{tag}", "grad.dx", f"{blk}.up")
                read(f"grad:{blk}.skip{tag}", f"grad.dskip{stop - 1}", f"{blk}.skip")
        # ---- stopped after bott, enc3, enc2
        for stop, (blk, pool) in ENC.items():
            step(stop=stop)
            read(f"grad:{blk}.y2", "grad.dy2", f"{blk}.y2")
            read(f"grad:{blk}.y1", "grad.da1", f"{blk}.y1")
            read(f"grad:{pool}", "grad.dx", pool)
            if blk == "bott":
                read("grad:bott.out", "grad.out", "bott.out")
    finally:
        for key, v in ((0, -1), (1, 0), (2, 1), (4, 1)):
            plan.debug_set(key, v)

    rows = stage_errors(engine, ref64.flat(), ref32.flat())
    print(f"\n{name}: per-voxel error of max|ref64| (gradients in backward order, then forward)")
    print(format_rows(rows))
    for k, a, b in rows:
        print(f"STAGE {name} {k} {a:.3e} {b:.3e}")
    bad = failing(rows)
    grads = [r for r in bad if r[0].startswith("grad:")]
    fwds = [r for r in bad if not r[0].startswith("grad:")]
    assert not bad, (f"{len(bad)} stages above max(8 x e_32, 2e-5)"
                     + (f"; first in backward order: {grads[0]}" if grads else "")
                     + (f"; first forward stage: {fwds[0]}" if fwds else ""))
