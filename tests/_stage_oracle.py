"""Per-voxel stages of the oracle's forward and backward (test infrastructure).

The parameter gradients that tests/_spff_checks.check_grads compares are sums over
every voxel: a backward pass that is wrong on a thin set of voxels (a last partial tile,
the last chunk of a split reduction, one (b, d) slab) moves them by far less than that
check's 1e-3 of the tensor's scale.  ``stage_grads`` runs one oracle step and keeps, per
voxel, the forward value and the gradient at every tensor the engine's backward holds in
a scratch view: each conv output (y1, y2), each pool output, each encoder block's
``_post`` output (the total of its skip and pool shares), each decoder block's two inputs
taken separately, and each block's output.  ``stage_errors`` compares an engine's views
with an fp64 run and reports, beside each, the fp32 oracle's own error -- the measure of
what fp32 arithmetic can give at that stage.

Keys: ``"<stage>"`` is a forward value, ``"grad:<stage>"`` the gradient at it; an engine
key may end in ``"@<tag>"`` (the same stage read in another run).  Stages: ``<blk>.y1``,
``<blk>.y2``, ``<blk>.out`` (after ``_post`` for enc1..3 and bott), ``pool1..3``,
``dec1..3.up`` (after any interpolation) and ``dec1..3.skip``.  Every tensor is channel
last, ``[B*D*H*W, C]``, float64.
"""
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from oracle import spff_oracle as O

BLOCKS = ("enc1", "enc2", "enc3", "bott", "dec3", "dec2", "dec1")


def _cl(t):
    """[B, C, D, H, W] -> float64 numpy [B*D*H*W, C]"""
    return t.detach().permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).double().cpu().numpy()


@dataclass
class StageRun:
    fwd: dict = field(default_factory=dict)        # stage -> [V, C]
    grad: dict = field(default_factory=dict)       # stage -> [V, C]
    shape: dict = field(default_factory=dict)      # stage -> (B, C, D, H, W)
    conv_in: dict = field(default_factory=dict)    # "<blk>.y1" / "<blk>.y2" -> the conv's input
    conv_w: dict = field(default_factory=dict)     # "<blk>.y1" / "<blk>.y2" -> its weight's key
    param_grads: dict = field(default_factory=dict)
    masks: dict = field(default_factory=dict)      # the run's own branches (none were forced)
    logits: np.ndarray = None
    loss: float = 0.0

    def flat(self):
        """The comparator's view: forward values and ``grad:`` entries in one dict."""
        out = dict(self.fwd)
        out.update({"grad:" + k: v for k, v in self.grad.items()})
        return out


def stage_grads(cfg, st, x, labels, masks=None, dtype=torch.float64, keep_inputs=False):
    """One ``O.fwd_bwd`` with every stage retained.  ``masks`` (as
    tests/_spff_checks.engine_branch_masks returns them) force the LeakyReLU signs and
    the pool argmaxes, as tests/_kink.forced_branches does; None leaves the oracle's own
    branches -- recorded in ``.masks``, to force on another run -- and the parameter
    gradients bitwise those of a plain ``O.fwd_bwd``.
    ``x`` / ``labels``: numpy arrays or tensors; ``st``: the state dict (numpy)."""
    a_, b_ = ("pre", "body") if cfg.novel else ("b1", "b2")
    x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    labels = torch.as_tensor(np.ascontiguousarray(labels) if isinstance(labels, np.ndarray)
                             else labels)
    kept = {}
    run = StageRun()
    count = {"pool": 0, "cat": 0}

    def keep(name, t):
        """t passes through a retained identity (a view: bitwise transparent)"""
        if not t.requires_grad:
            return t
        t = t.view_as(t)
        t.retain_grad()
        kept[name] = t
        return t

    def conv_in_lrelu(P, pre, inp, ksd):
        blk, tag = pre.rsplit(".", 1)
        name = f"{blk}.{'y1' if tag == a_ else 'y2'}"
        y = F.conv3d(inp, P[pre + ".0.weight"], None, padding=(ksd // 2, 1, 1))
        y = keep(name, y)
        if keep_inputs:
            run.conv_in[name] = inp.detach()
            run.conv_w[name] = pre + ".0.weight"
        r = F.instance_norm(y, weight=P[pre + ".1.weight"], bias=P[pre + ".1.bias"], eps=1e-5)
        if masks is None:
            run.masks[pre] = (r.detach() > 0).contiguous()
            return F.leaky_relu(r, 0.01)
        # (contiguous: see engine_branch_masks on this torch build's instance_norm backward)
        return torch.where(masks[pre].contiguous(), r, 0.01 * r)

    def maxpool(t):
        k = count["pool"] % 3
        count["pool"] += 1
        B_, C_, D_, H_, W_ = t.shape
        v = t[..., :H_ // 2 * 2, :W_ // 2 * 2].reshape(B_, C_, D_, H_ // 2, 2, W_ // 2, 2)
        v = v.permute(0, 1, 2, 3, 5, 4, 6).reshape(B_, C_, D_, H_ // 2, W_ // 2, 4)
        if masks is None:
            run.masks[f"pool{k + 1}"] = v.detach().argmax(-1)
            return keep(f"pool{k + 1}", orig["maxpool"](t))
        return keep(f"pool{k + 1}", v.gather(-1, masks[f"pool{k + 1}"].unsqueeze(-1)).squeeze(-1))

    def _post(P, t, stage, cfg_):
        return keep(f"{BLOCKS[stage]}.out", orig["_post"](P, t, stage, cfg_))

    def _cat(up, skip):
        name = ("dec3", "dec2", "dec1")[count["cat"] % 3]
        count["cat"] += 1
        if up.shape[-3:] != skip.shape[-3:]:
            up = F.interpolate(up, size=skip.shape[-3:], mode="trilinear", align_corners=False)
        return torch.cat([keep(name + ".up", up), keep(name + ".skip", skip)], dim=1)

    def novel_block(P, pre, t, cfg_):
        o = orig["novel_block"](P, pre, t, cfg_)
        return keep(pre + ".out", o) if pre.startswith("dec") else o

    hooks = {"conv_in_lrelu": conv_in_lrelu, "maxpool": maxpool, "_post": _post, "_cat": _cat,
             "novel_block": novel_block}
    orig = {k: getattr(O, k) for k in hooks}
    for k, fn in hooks.items():
        setattr(O, k, fn)
    try:
        P = O.params_from_state({k: v for k, v in st.items() if not k.endswith("._mask")},
                                dtype=dtype)
        logits, loss, _ce, _dice = O.fwd_bwd(P, x.to(dtype), labels, cfg)
    finally:
        for k, fn in orig.items():
            setattr(O, k, fn)
    for name, t in kept.items():
        run.fwd[name] = _cl(t)
        run.grad[name] = _cl(t.grad)
        run.shape[name] = tuple(t.shape)
    run.param_grads = {k: v.grad.detach().clone() for k, v in P.items() if v.grad is not None}
    run.logits = _cl(logits)
    run.loss = float(loss)
    return run


def stage_order(key):
    """Sort key: the gradients in backward order (dec1 first, enc1 last), then the forward
    values in forward order."""
    name = key.split("@")[0]
    is_grad = name.startswith("grad:")
    name = name[5:] if is_grad else name
    if name.startswith("pool"):
        blk, part = "enc%d" % int(name[4:]), "pool"
    else:
        blk, part = name.split(".")
    # forward order within a block; the pool follows its encoder block's output
    within = ("up", "skip", "y1", "y2", "out", "pool").index(part)
    fwd = BLOCKS.index(blk) * 8 + within
    return (0, -fwd) if is_grad else (1, fwd)


def stage_errors(engine, ref64, ref32):
    """rows (stage, e_gpu, e_32), sorted by ``stage_order``: for every key of ``engine``,
    max|a - ref64| / max|ref64| over the whole tensor (no voxel excluded) for the engine's
    tensor and for the fp32 oracle's."""
    rows = []
    for key in sorted(engine, key=stage_order):
        name = key.split("@")[0]
        r64 = np.asarray(ref64[name], np.float64)
        a = np.asarray(engine[key], np.float64).reshape(r64.shape)
        scale = max(float(np.abs(r64).max()), 1e-300)
        e_gpu = float(np.abs(a - r64).max()) / scale
        e_32 = float(np.abs(np.asarray(ref32[name], np.float64) - r64).max()) / scale
        rows.append((key, e_gpu, e_32))
    return rows


FACTOR, FLOOR = 8.0, 2e-5


def stage_bar(e_32):
    """8 x the fp32 oracle's own error (check_grads' factor), at least the 2e-5 of max that
    test_conv3d_fwd_dgrad_wgrad accepts of one fp32-MFMA conv."""
    return max(FACTOR * e_32, FLOOR)


def failing(rows):
    return [(k, a, b) for k, a, b in rows if not a <= stage_bar(b)]


def format_rows(rows):
    return "\n".join(f"  {k:28s} gpu {a:.2e}  fp32-oracle {b:.2e}"
                     f"{'' if a <= stage_bar(b) else '  <-- above the bar'}" for k, a, b in rows)
