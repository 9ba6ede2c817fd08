"""Loss and metrics of the SPFF hot path (mirror of innovative3D/helpers.py).

* ``ce_plus_macro_dice_loss`` (helpers.py:797-803): one fused HIP kernel --
  softmax-CE with ignore_index, its gradient, the argmax confusion matrix and
  the hard macro-Dice term, all on the device (no host syncs).  As in the
  reference, the Dice term is a constant: the gradient is the CE gradient only.
* ``macro_dice_loss`` (helpers.py:782-795) and ``per_class_metrics_3d/2d``
  (helpers.py:668-725, 728-779): the confusion counts come from the HIP kernel
  (one device->host copy); the NaN / absent-class algebra runs on the host
  exactly as the reference does it.
* ``ranking_metrics``: the test-only PR-AUC / ROC-AUC / IoU / precision block of
  ``BaseLitModel._shared_step`` (models.py:510-584) -- the ranking part is the exact
  segmented sort + scan of csrc/rank.hip instead of scikit-learn on the host.
* ``prediction_views`` / ``render_overlays`` / ``write_png``: the qualitative figures of
  train.py:649-671 and 1071-1119 -- class maps, confidence and the depth-wise maximum of
  the softmax come from csrc/views.hip in one read of the logits; the five panels are
  composed on the device and written as a PNG with zlib (no matplotlib).
* ``predict_tiled``: sliding-window inference with Gaussian blending for any module that
  returns [B, K, D, H, W] logits -- window gather, blend, class map and counts are the
  kernels of csrc/tile.hip; the window geometry is innovative3D/tiling.py.

``LOSS_REGISTRY``: ``ce_plus_macro_dice`` is the SPFF path's loss (config.LOSS_NAME is never
read by it); ``dice_ce_nnunet`` is models.dice_ce_loss on the soft-Dice loss driver;
``focal_plus_gradient`` raises, because the reference's own function cannot run.
"""
from __future__ import annotations

import warnings
from typing import Optional

import numpy as np
import torch

from . import _engine as E

__all__ = ["ce_plus_macro_dice_loss", "macro_dice_loss", "per_class_metrics_3d",
           "per_class_metrics_2d", "metrics_from_confusion", "ce_dice_with_confusion",
           "ce_dice_parts", "dice_loss_from_confusion_t", "ranking_metrics",
           "iou_precision_from_confusion", "dice_ce_loss_adapter", "LOSS_REGISTRY",
           "prediction_views", "render_overlays", "write_png", "default_palette", "color_table",
           "main_logits", "predict_tiled"]


def _logits_cl(logits: torch.Tensor) -> torch.Tensor:
    """[B,K,D,H,W] (or [B,K,H,W]) -> channel-last contiguous; free for the
    engine's channels_last_3d logits."""
    if logits.ndim == 4:
        logits = logits.unsqueeze(2)
    if logits.ndim != 5:
        raise ValueError(f"expected [B,K,D,H,W] logits, got {tuple(logits.shape)}")
    return logits.permute(0, 2, 3, 4, 1).contiguous()


class _DeviceLoss(torch.autograd.Function):
    """Base of the losses whose HIP forward pass also writes dloss/dlogits.  A subclass
    gives ``WHAT`` (its name in messages) and ``run(logits_cl, labels, *args)`` ->
    (dlogits_cl, loss, *extras): the call into the engine on channel-last logits.  apply
    takes (logits [B,K,D,H,W] or [B,K,H,W], labels, *args) and returns loss, or
    (loss, *extras) with the extras carrying no gradient."""

    WHAT = "device loss"

    @classmethod
    def forward(cls, ctx, logits, labels, *args):
        dl, loss, *extras = cls.run(_logits_cl(logits), labels, *args)
        ctx.dl, ctx.ndim, ctx.nin = dl, logits.ndim, 2 + len(args)
        ctx.mark_non_differentiable(*extras)
        return (loss, *extras) if extras else loss

    @classmethod
    def backward(cls, ctx, g, *_gextras):
        # scaled in place (no second logits-sized buffer: 7 GB at 5 x 512^3) and handed
        # out exactly once; a retained-graph second backward would see a scaled tensor
        dl = ctx.dl
        if dl is None:
            raise RuntimeError(f"{cls.WHAT}: backward ran twice through the same graph "
                               "(retain_graph); recompute the loss for a second backward")
        ctx.dl = None
        E.scale_(dl, g.reshape(1))
        d = dl.permute(0, 4, 1, 2, 3)
        if ctx.ndim == 4:
            d = d.squeeze(2)
        return (d,) + (None,) * (ctx.nin - 1)


class _CEDice(_DeviceLoss):
    """(logits, labels, K, ignore_index, smooth, count_override) -> (loss, conf, ce):
    loss = ce + 0.5 * hard-Dice term (out4[1]); conf [K, K+1] and the CE share ce (out4[0])
    carry no gradient."""

    WHAT = "ce_plus_macro_dice_loss"

    @staticmethod
    def run(lcl, labels, *args):
        out4, dl, conf = E.ce_dice_forward(lcl, labels, *args)
        return dl, out4[1], conf, out4[0]


def ce_dice_parts(logits, labels, num_classes, ignore_index=255, smooth=1e-6,
                  count_override: Optional[torch.Tensor] = None):
    """(loss, conf[K, K+1], ce) on the device with no host sync: loss as
    ce_plus_macro_dice_loss (differentiable through the CE only, as in the
    reference), conf[pred, label] of the argmax, ce = the CE term (with
    ``count_override`` = the global valid count, this rank's share of it)."""
    E.require_device(logits, "ce_plus_macro_dice_loss")
    if labels.ndim == logits.ndim and labels.shape[1] == 1:
        labels = labels[:, 0]
    return _CEDice.apply(logits, labels, int(num_classes), int(ignore_index), float(smooth),
                         count_override)


def ce_dice_with_confusion(logits, labels, num_classes, ignore_index=255, smooth=1e-6,
                           count_override: Optional[torch.Tensor] = None):
    """(loss, conf[K, K+1]) -- loss as ce_plus_macro_dice_loss; conf[pred, label]."""
    loss, conf, _ce = ce_dice_parts(logits, labels, num_classes, ignore_index, smooth,
                                    count_override)
    return loss, conf


def ce_plus_macro_dice_loss(logits, labels, num_classes, ignore_index=255, smooth=1e-6):
    """F.cross_entropy(ignore_index) + 0.5 * macro_dice_loss (helpers.py:797-803)."""
    loss, _conf = ce_dice_with_confusion(logits, labels, num_classes, ignore_index, smooth)
    return loss


def _conf_np(logits, labels, num_classes, ignore_index):
    conf = E.confusion(_logits_cl(logits.detach()), labels, int(num_classes), ignore_index)
    return conf.cpu().numpy()


def macro_dice_loss(logits, labels, num_classes, ignore_index=255, smooth=1e-6):
    """1 - mean_{c>=1} hard Dice, plain mean (no NaN skipping), python float."""
    conf = _conf_np(logits, labels, num_classes, ignore_index)
    return dice_loss_from_confusion(conf, num_classes, smooth)


def dice_loss_from_confusion(conf, num_classes, smooth=1e-6):
    """macro_dice_loss (helpers.py:782-795) from confusion counts conf[pred, label]
    (a column K of out-of-range labels, if present, counts as fp only)."""
    K = int(num_classes)
    vals = []
    for c in range(1, K):
        tp = int(conf[c, c])
        fp = int(conf[c, :].sum()) - tp
        fn = int(conf[:K, c].sum()) - tp
        vals.append((2 * tp + smooth) / (2 * tp + fp + fn + smooth))
    return 1.0 - (float(np.mean(vals)) if vals else 1.0)


def dice_loss_from_confusion_t(conf: torch.Tensor, num_classes: int,
                               smooth: float = 1e-6) -> torch.Tensor:
    """dice_loss_from_confusion with torch ops on conf's device (fp64, no host sync).
    conf: [K, K+1] or [K, K] counts (int64 or exactly-integer fp64)."""
    K = int(num_classes)
    c = conf.to(torch.float64)
    if K < 2:
        return torch.zeros((), dtype=torch.float64, device=conf.device)
    tp = torch.diagonal(c[:, :K])[1:]
    fp = c[1:K, :].sum(1) - tp
    fn = c[:K, 1:K].sum(0) - tp
    return 1.0 - ((2 * tp + smooth) / (2 * tp + fp + fn + smooth)).mean()


def metrics_from_confusion(conf: np.ndarray, K: int, n_voxels: int, smooth: float = 1e-6):
    """helpers.py:668-725 on counts.  conf is [K, K+1] (column K: labels not in
    [0,K), which count as 'not class c' for every c).  Reference quirk kept:
    tn uses the masked pred_c/label_c, so ignored voxels are true negatives
    (helpers.py:689) -> n_voxels = ALL voxels of the batch."""
    conf = np.asarray(conf, dtype=np.int64)
    dice_l, sens_l, spec_l = [], [], []
    for c in range(K):
        tp = int(conf[c, c])
        fp = int(conf[c, :].sum()) - tp
        fn = int(conf[:K, c].sum()) - tp
        tn = int(n_voxels) - tp - fp - fn
        if (tp + fn) == 0 and fp == 0:
            dice = float("nan"); sens = float("nan")
        else:
            dice = (2 * tp + smooth) / (2 * tp + fp + fn + smooth)
            sens = (tp + smooth) / (tp + fn + smooth) if (tp + fn) > 0 else float("nan")
        spec = (tn + smooth) / (tn + fp + smooth) if (tn + fp) > 0 else float("nan")
        dice_l.append(dice); sens_l.append(sens); spec_l.append(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        nm = lambda v: float(np.nanmean(v[1:])) if len(v) > 1 else float("nan")  # noqa: E731
        macro_dice, macro_sens, macro_spec = nm(dice_l), nm(sens_l), nm(spec_l)
    tp_sum = sum(int(conf[c, c]) for c in range(1, K))
    fp_sum = sum(int(conf[c, :].sum()) - int(conf[c, c]) for c in range(1, K))
    fn_sum = sum(int(conf[:K, c].sum()) - int(conf[c, c]) for c in range(1, K))
    tn_sum = int(conf[0, 0])
    dd = 2 * tp_sum + fp_sum + fn_sum
    micro_dice = (2 * tp_sum + smooth) / (dd + smooth) if dd > 0 else float("nan")
    micro_sens = (tp_sum + smooth) / (tp_sum + fn_sum + smooth) if (tp_sum + fn_sum) > 0 else float("nan")
    micro_spec = (tn_sum + smooth) / (tn_sum + fp_sum + smooth) if (tn_sum + fp_sum) > 0 else float("nan")
    return (dice_l, sens_l, spec_l, macro_dice, macro_sens, macro_spec, micro_dice, micro_sens,
            micro_spec)


def per_class_metrics_3d(preds, labels, num_classes, smooth=1e-6, ignore_index=None):
    """Returns the reference 9-tuple (dice/sens/spec lists, macro_*, micro_*)."""
    conf = _conf_np(preds, labels, num_classes, ignore_index)
    return metrics_from_confusion(conf, int(num_classes), int(labels.numel()), smooth)


def per_class_metrics_2d(preds, labels, num_classes, smooth=1e-6, ignore_index=None):
    return per_class_metrics_3d(preds, labels, num_classes, smooth, ignore_index)


def _nanmean_fg(vals):
    """models.py:546: nanmean over the classes 1..K-1 (over the one class when K == 1)."""
    v = np.asarray(vals[1:] if len(vals) > 1 else vals, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(np.nanmean(v)) if v.size else float("nan")


def iou_precision_from_confusion(conf, num_classes):
    """jaccard_score / precision_score(zero_division=0) of models.py:537-550, 566-567 on
    confusion counts conf[pred, label] taken WITHOUT an ignore mask ([K, K+1]: column K
    holds the labels outside [0, K), 255 included, which are "not class c" for every c
    while their predictions still count).  Returns (iou[K], precision[K], iou_macro,
    precision_macro, iou_micro, precision_micro).  Per class: IoU is NaN when the class is
    absent from labels and predictions; precision is 0 when only the prediction is absent
    and NaN when both are.  The micro forms over the classes 1..K-1 are unguarded as in
    the reference: an empty denominator gives 0 (sklearn's zero_division), K < 2 gives NaN."""
    K = int(num_classes)
    conf = np.asarray(conf, dtype=np.int64)
    iou, prec = [], []
    tp_s = fp_s = fn_s = 0
    for c in range(K):
        tp = int(conf[c, c])
        fp = int(conf[c, :].sum()) - tp
        fn = int(conf[:K, c].sum()) - tp
        if c >= 1:
            tp_s, fp_s, fn_s = tp_s + tp, fp_s + fp, fn_s + fn
        present = (tp + fp + fn) > 0
        iou.append(tp / (tp + fp + fn) if present else float("nan"))
        prec.append((tp / (tp + fp) if (tp + fp) > 0 else 0.0) if present else float("nan"))
    if K > 1:
        iou_micro = tp_s / (tp_s + fp_s + fn_s) if (tp_s + fp_s + fn_s) > 0 else 0.0
        prec_micro = tp_s / (tp_s + fp_s) if (tp_s + fp_s) > 0 else 0.0
    else:
        iou_micro = prec_micro = float("nan")
    return iou, prec, _nanmean_fg(iou), _nanmean_fg(prec), iou_micro, prec_micro


def ranking_metrics(logits, labels, num_classes, per_sample=False):
    """The test-only metrics of BaseLitModel._shared_step (models.py:510-584) and of the
    per-volume rows of train.py:773-798, on the device: the exact, tie-aware PR-AUC and
    ROC-AUC of the fp32 softmax (csrc/rank.hip) and IoU / precision from the argmax
    confusion kernel run without an ignore mask.  Returns a dict with ``pr_auc``,
    ``roc_auc``, ``iou`` and ``precision`` as lists of K floats and their ``_macro`` /
    ``_micro`` forms, or -- ``per_sample`` -- as [B][K] lists only.  One device-to-host
    copy per call (per sample for the confusion counts)."""
    E.require_device(logits, "ranking_metrics")
    K = int(num_classes)
    if labels.ndim == logits.ndim and labels.shape[1] == 1:
        labels = labels[:, 0]
    lcl = _logits_cl(logits.detach())
    B = lcl.shape[0]
    labels = labels.to(lcl.device).long().reshape(B, -1)
    auc = E.rank_auc(lcl, labels, K, True, per_sample).cpu().numpy()
    if per_sample:
        auc = auc.reshape(B, K, 4)
        ip = [iou_precision_from_confusion(E.confusion(lcl[b], labels[b], K, None).cpu().numpy(), K)
              for b in range(B)]
        return {"pr_auc": [[float(v) for v in auc[b, :, 0]] for b in range(B)],
                "roc_auc": [[float(v) for v in auc[b, :, 1]] for b in range(B)],
                "iou": [p[0] for p in ip], "precision": [p[1] for p in ip]}
    iou, prec, iou_ma, prec_ma, iou_mi, prec_mi = iou_precision_from_confusion(
        E.confusion(lcl, labels, K, None).cpu().numpy(), K)
    pr = [float(v) for v in auc[:K, 0]]
    roc = [float(v) for v in auc[:K, 1]]
    return {"pr_auc": pr, "roc_auc": roc, "iou": iou, "precision": prec,
            "pr_auc_macro": _nanmean_fg(pr), "roc_auc_macro": _nanmean_fg(roc),
            "iou_macro": iou_ma, "precision_macro": prec_ma,
            "pr_auc_micro": float(auc[K, 0]), "roc_auc_micro": float(auc[K, 1]),
            "iou_micro": iou_mi, "precision_micro": prec_mi}


def main_logits(out):
    """The tensor a figure shows of whatever ``model(x)`` returns (train.py:1029-1051): the
    tensor itself, a dict's ``"logits"``, or -- deep supervision -- the tensor of a tuple or
    list with the largest spatial volume."""
    if torch.is_tensor(out):
        return out
    if isinstance(out, dict) and torch.is_tensor(out.get("logits")):
        return out["logits"]
    if isinstance(out, (tuple, list)):
        ts = [t for t in out if torch.is_tensor(t)]
        if ts:
            return max(ts, key=lambda t: int(np.prod(t.shape[2:])) if t.ndim >= 4 else 0)
    raise TypeError(f"no logits tensor in a model output of type {type(out).__name__}")


@torch.no_grad()
def predict_tiled(model, x, roi, overlap=0.5, blend="gaussian", sigma_scale=0.125,
                  blend_of="logits", window_batch=1, mirror_axes=(), labels=None,
                  ignore_index=None, return_scores=False, *, forward_cl=None):
    """Sliding-window inference: ``model`` runs on overlapping windows of
    ``roi`` = (D, H, W) voxels (clamped to the volume) of x [B, C, D, H, W], ``window_batch``
    windows per forward, and the window outputs -- the logits, or with ``blend_of="probs"``
    their fp32 softmax -- are blended on the device (csrc/tile.hip) with a window-centred
    ``gaussian`` or a ``constant`` weight; ``mirror_axes``, a subset of (0, 1, 2) = (D, H, W),
    adds one pass over all windows per subset of mirrored axes.  Volumes are processed one
    after another.  Returns like ``predict``: the class mask uint8 [B, D, H, W] (the first
    maximum of the blend), then with ``labels`` [B, D, H, W] the [K, K + 1] int64 confusion
    counts summed over the batch (``ignore_index`` None: no voxel masked), then with
    ``return_scores`` the normalised blend [B, K, D, H, W].

    ``model(x)`` must return [B, K, D, H, W] logits (or what main_logits finds them in).
    One staging tensor and one window-output buffer serve every window; a partial last batch
    repeats its last window in the unused slots, which the blend leaves out.
    ``forward_cl(stage, out)``: the engine modules' own forward, channel-last into ``out``."""
    from . import tiling as T
    E.require_device(x, "predict_tiled")
    if x.ndim != 5:
        raise ValueError(f"predict_tiled: expected x [B, C, D, H, W], got {tuple(x.shape)}")
    if blend_of not in ("logits", "probs"):
        raise ValueError(f"blend_of={blend_of!r}: expected 'logits' or 'probs'")
    x = x.detach().float()
    dev = x.device
    B, C, D, H, W = (int(v) for v in x.shape)
    r = T.clamp_roi((D, H, W), roi)
    table = T.window_table((D, H, W), r, overlap, mirror_axes)
    wb = int(window_batch)
    spans = T.batches(len(table), wb)
    weights = tuple(torch.from_numpy(T.axis_weights(ri, blend, sigma_scale)).to(dev) for ri in r)
    norms = None
    if return_scores:
        norms = tuple(torch.from_numpy(v).to(dev)
                      for v in T.norm_vectors((D, H, W), r, overlap, blend, sigma_scale))
    if labels is not None:
        labels = labels.detach().to(dev)
        if labels.ndim == 5 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if tuple(labels.shape) != (B, D, H, W):
            raise ValueError(f"predict_tiled: labels {tuple(labels.shape)} do not match the "
                             f"volumes {(B, D, H, W)}")
    stage = torch.empty((wb, C) + r, dtype=torch.float32, device=dev)
    mask = torch.empty((B, D, H, W), dtype=torch.uint8, device=dev)
    tiles = acc = scores = conf = None
    for b in range(B):
        vol = x[b].contiguous()
        if acc is not None:
            acc.zero_()
        for i0, i1 in spans:
            rows = table[i0:i1]
            if i1 - i0 < wb:  # the partial last batch: same plan, the last window repeated
                rows = np.concatenate([rows, np.repeat(rows[-1:], wb - (i1 - i0), axis=0)])
            E.tile_gather(vol, rows, r, out=stage)
            if forward_cl is not None:
                tiles = forward_cl(stage, tiles)
            else:
                lg = main_logits(model(stage))
                if lg.ndim != 5 or tuple(lg.shape[2:]) != r or lg.shape[0] != wb:
                    raise ValueError(f"predict_tiled: the model returned {tuple(lg.shape)} for "
                                     f"windows {tuple(stage.shape)}")
                if tiles is None:
                    tiles = torch.empty((wb,) + r + (int(lg.shape[1]),), dtype=torch.float32,
                                        device=dev)
                tiles.copy_(lg.detach().permute(0, 2, 3, 4, 1))
            if acc is None:
                K = int(tiles.shape[-1])
                acc = torch.zeros((D, H, W, K), dtype=torch.float32, device=dev)
                if return_scores:
                    scores = torch.empty((B, D, H, W, K), dtype=torch.float32, device=dev)
            E.tile_accumulate(tiles, table[i0:i1], weights, acc, softmax=blend_of == "probs")
        _m, cf, _s = E.tile_finalize(acc, norms, len(T.flip_passes(mirror_axes)),
                                     None if labels is None else labels[b], ignore_index,
                                     scores=scores[b] if return_scores else False, mask=mask[b])
        if cf is not None:
            conf = cf if conf is None else conf + cf
    out = (mask,)
    if labels is not None:
        out += (conf,)
    if return_scores:
        out += (scores.permute(0, 4, 1, 2, 3),)
    return out[0] if len(out) == 1 else out


def prediction_views(logits):
    """_prediction_views_and_mip (train.py:649-671) for every sample of logits [B, K, D, H, W],
    or [B, K, H, W] (the reference's 2-D branch: D = 1, all three class maps are the centre
    one), on the device (csrc/views.hip: one read of the logits, no copy to the host).
    Returns ``center_pred, summary_pred, alpha_center, mip_pred`` in the reference's order:
    uint8 class maps and the fp32 confidence, each [B, H, W]; ``summary_pred`` is
    ``mip_pred``, as in the reference."""
    E.require_device(logits, "prediction_views")
    center_pred, alpha_center, _mip_prob, mip_pred = E.pred_views(_logits_cl(logits.detach()))
    return center_pred, mip_pred, alpha_center, mip_pred


def default_palette(num_classes: int) -> dict:
    """{class: (r, g, b)} for classes 0 .. K-1: class 0 black, the others evenly spaced hues
    at full saturation and value."""
    import colorsys
    K = int(num_classes)
    pal = {0: (0, 0, 0)}
    for c in range(1, K):
        r, g, b = colorsys.hsv_to_rgb((c - 1) / max(1, K - 1), 1.0, 1.0)
        pal[c] = (int(round(255 * r)), int(round(255 * g)), int(round(255 * b)))
    return pal


def color_table(colors, num_classes: int) -> torch.Tensor:
    """uint8 [256, 3] (host) from a ``{class: (r, g, b)}`` dict, the shape config.label_colors
    has; ``None``: default_palette.  A class without an entry stays black."""
    colors = default_palette(num_classes) if colors is None else colors
    tab = np.zeros((256, 3), dtype=np.uint8)
    for c, col in colors.items():
        if not 0 <= int(c) < 256 or len(col) != 3 or not all(0 <= int(v) <= 255 for v in col):
            raise ValueError(f"colour table entry {c!r}: {col!r}")
        tab[int(c)] = [int(v) for v in col]
    return torch.from_numpy(tab)


def render_overlays(x, labels, logits, colors=None, max_items=2):
    """The five panels of the reference's overlay figure (train.py:1071-1119: original,
    ground truth, centre prediction, prediction over the MIP, confidence-weighted overlay)
    for the first ``max_items`` samples, as one uint8 strip [n, H, 5 W, 3] on the device.
    x [B, C, D, H, W] (or [B, C, H, W]: the frame C // 2, train.py:620-622), labels
    [B, D, H, W], [B, 1, D, H, W], [B, H, W] or None, logits whatever the model returned.
    ``colors``: a ``{class: (r, g, b)}`` dict; None: default_palette."""
    logits = main_logits(logits)
    E.require_device(logits, "render_overlays")
    n = max(1, min(int(max_items), int(logits.shape[0])))
    lcl = _logits_cl(logits.detach()[:n])
    _B, D, H, W, K = lcl.shape
    x = x.detach()[:n].to(lcl.device)
    if x.ndim == 4:
        x = x[:, x.shape[1] // 2][:, None, None]
    if x.ndim != 5 or tuple(x.shape[-2:]) != (H, W):
        raise ValueError(f"input {tuple(x.shape)} does not match logits {tuple(logits.shape)}")
    yc = None
    if labels is not None:
        y = labels.detach()[:n]
        if y.ndim == 5 and y.shape[1] == 1:
            y = y[:, 0]
        if y.ndim == 4:
            y = y[:, y.shape[1] // 2]
        if y.ndim != 3 or tuple(y.shape[-2:]) != (H, W):
            raise ValueError(f"labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        yc = y.to(lcl.device).long()
    center_pred, alpha_center, _mip_prob, mip_pred = E.pred_views(lcl)
    center, mip, rng = E.input_views(x)
    tab = color_table(colors, K).to(lcl.device)
    return E.overlay_rgb(center, mip, rng, yc, center_pred, mip_pred, alpha_center, tab, K)


def write_png(path, rgb):
    """An 8-bit RGB PNG of ``rgb`` (uint8 [H, W, 3], tensor or array) with zlib and struct
    only; written under a temporary name and moved into place (train.py:894-900), so a
    reader never sees half a file."""
    import os
    import pathlib
    import struct
    import zlib
    if torch.is_tensor(rgb):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or 0 in rgb.shape:
        raise ValueError(f"write_png: expected uint8 [H, W, 3], got {rgb.dtype} {rgb.shape}")
    h, w, _ = rgb.shape
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)  # filter type 0 in front of every row
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(tag, data):
        return (struct.pack(">I", len(data)) + tag + data +
                struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF))

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
           chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))
    path = pathlib.Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + ".part.png")
    tmp.write_bytes(png)
    os.replace(tmp, path)
    return path


def fast_simple_metrics() -> bool:
    """FAST_SIMPLE_METRICS=1 (train.py:24, 106-108, 120): skip the ranking metrics of the
    test step and of test_details.csv."""
    import os
    return os.environ.get("FAST_SIMPLE_METRICS", "0").strip().lower() in ("1", "true", "yes", "on")


def dice_ce_loss_adapter(logits, labels, num_classes, ignore_index):
    """helpers.py:947-949: models.dice_ce_loss with its own weights and background setting."""
    from .models import dice_ce_loss as _dice_ce
    return _dice_ce(logits, labels, num_classes, ignore_index=ignore_index)


def _focal_plus_gradient(*a, **k):
    raise NotImplementedError(
        "loss 'focal_plus_gradient': the reference's focal_plus_gradient_loss raises IndexError "
        "in _spatial_grad_3d (its shift writes pad[2 * dim + 1] of a six-entry list with dim = "
        "3, 4), so there is no behaviour to reproduce")


LOSS_REGISTRY = {
    "ce_plus_macro_dice": lambda logits, labels, nc, ignore_index: ce_plus_macro_dice_loss(
        logits, labels, nc, ignore_index=ignore_index),
    "focal_plus_gradient": _focal_plus_gradient,
    "dice_ce_nnunet": lambda logits, labels, nc, ignore_index: dice_ce_loss_adapter(
        logits, labels, nc, ignore_index),
}


# ------------------------------------------------------------- data path ---
# helpers.py:125-211 / 280-289, device-side: see
# innovative3D/datasets.py and csrc/data.hip.
def is_pixel_in_ellipse(x, y, roi):
    """helpers.py:125-129."""
    cx, cy = roi[0] + roi[2] / 2, roi[1] + roi[3] / 2
    a, b = roi[2] / 2, roi[3] / 2
    return ((x - cx) ** 2) / (a * a) + ((y - cy) ** 2) / (b * b) <= 1


def generate_cumulative_grid_sizes(num_images, num_grid_sizes=10, cumulative_percentage=0.2):
    """helpers.py:280-289 (module-level random, same draws)."""
    import random
    per = int(num_images * cumulative_percentage)
    out = []
    for gs in range(1, num_grid_sizes + 1):
        out.extend([gs] * per)
    rem = num_images - len(out)
    if rem > 0:
        out.extend(random.choices(range(1, num_grid_sizes + 1), k=rem))
    random.shuffle(out)
    return out


def read_dicom_frames(path):
    """Decoded frames [n, h, w] of one DICOM file: ``pydicom.dcmread(path).pixel_array`` as
    helpers.py:190-191 when pydicom is installed, else the native reader (innovative3D/dicom.py:
    uncompressed transfer syntaxes; a compressed one raises NotImplementedError)."""
    try:
        import pydicom
    except ImportError:
        from .dicom import pixel_array
        return pixel_array(path)
    return pydicom.dcmread(path).pixel_array


def create_image_and_labels_for_dataset(cfg, num_frames, frames_reader=None, device=None):
    """helpers.py:132-211 on the device: every DICOM under cfg["dir"] -> frames resized to
    IMAGE_HEIGHT x IMAGE_WIDTH (antialiased bilinear, TF.resize) and the ellipse-ROI label
    map (later ROIs overwrite).  Returns (images [N,F,H,W] fp32, labels [N,F,H,W] int64) on
    the device.  A list of configs is concatenated, as in the reference."""
    import os
    from pathlib import Path
    from .config import IMAGE_HEIGHT, IMAGE_WIDTH, global_label_names
    if isinstance(cfg, (list, tuple)):
        parts = [create_image_and_labels_for_dataset(c, num_frames, frames_reader, device)
                 for c in cfg]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    dev = device or torch.device("cuda")
    folder = os.path.expanduser(os.path.expandvars(str(Path(cfg["dir"]).resolve())))
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"Images folder not found or not a directory: {folder}")
    paths = []
    for root, _, files in os.walk(folder):
        paths += [os.path.join(root, f) for f in files if f.lower().endswith((".dcm", ".dicom"))]
    if not paths:
        raise FileNotFoundError(f"No DICOM files (.dcm/.dicom) found under: {folder}")
    sx, sy = IMAGE_WIDTH / 1300.0, IMAGE_HEIGHT / 1300.0
    ox, oy = cfg["offset"]
    rois = []
    for (x, y, w, h, lab_str) in cfg["original_rois"]:
        lab = next((i for i, n in global_label_names.items() if n == lab_str), 0)
        rois.append((int((x + ox) * sx), int((y + oy) * sy), int(w * sx), int(h * sy), lab))
    rois_t = torch.tensor(rois, dtype=torch.int32).reshape(-1, 5).to(dev)
    reader = frames_reader or read_dicom_frames
    imgs, lbls = [], []
    for fn in paths:
        frames = np.asarray(reader(fn))
        n = min(frames.shape[0], num_frames)
        fr = torch.from_numpy(frames[:n].astype(np.float32)).to(dev)
        imgs.append(E.resize_bilinear_aa(fr, IMAGE_HEIGHT, IMAGE_WIDTH))
        lbls.append(E.rasterize_ellipses(rois_t, n, IMAGE_HEIGHT, IMAGE_WIDTH))
    return torch.stack(imgs), torch.stack(lbls)
