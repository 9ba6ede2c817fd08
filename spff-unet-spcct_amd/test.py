#!/usr/bin/env python3
"""Evaluation entry point of the MI355X engine, mirroring the parts of the
reference's test.py that touch the model (test.py:98-113 checkpoint lookup,
548-579 state-dict key alignment, 208-243 per-class aggregation over seeds):

  for each variant in VARIANTS (INNOVATIVE3D_VARIANT honoured) and seed in SEEDS:
  load best-*.ckpt (newest) or last.ckpt from CHECKPOINT_DIR/<model>/seed<k>/,
  run the engine on the test volumes, write test_details.csv (per volume and
  class: dice / sensitivity / specificity from the fused confusion kernel, and
  precision / IoU / PR-AUC / ROC-AUC from helpers.ranking_metrics unless
  FAST_SIMPLE_METRICS=1), and
  aggregate mean +- std over seeds into analysis/per_class_summary.csv -- the
  table the reference turns into heatmaps.

``--overlays N`` also draws the reference's qualitative overlays (test.py:581-744) for the
first N test volumes of every evaluated checkpoint into
<out>/overlays/<model>_seed<k>_case<i>.png: class maps, confidence and the softmax's
depth-wise maximum are formed on the device (csrc/views.hip), the five panels too, and the
PNG is written with zlib.  The other plots (heatmaps, Bland-Altman, violins, montages) are
host-side matplotlib drawings of numbers that are all in the CSVs written here.

``--roi D H W`` evaluates every variant by sliding-window inference (helpers.predict_tiled):
the network runs on overlapping windows of that size (``--overlap``, ``--window-batch`` per
forward, ``--mirror AXES`` for test-time mirroring), the window logits are blended with a
Gaussian weight on the device (csrc/tile.hip), and the metrics come from the blend.
"""
from __future__ import annotations

import argparse
import csv
import os
import pathlib
import statistics
import sys
from typing import Dict, Optional

HERE = pathlib.Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))

import torch  # noqa: E402

from innovative3D import config as C  # noqa: E402
from innovative3D import helpers as Hh  # noqa: E402
from innovative3D import models as M  # noqa: E402
from innovative3D.synthetic import SyntheticSPCCT  # noqa: E402
from train import Settings, _build_lit  # noqa: E402


def find_best_or_last_ckpt(ckpt_dir: pathlib.Path, model: str, seed: int) -> Optional[pathlib.Path]:
    """test.py:105-111: newest best-*.ckpt, else last.ckpt."""
    root = ckpt_dir / model / f"seed{seed}"
    bests = sorted(root.glob("best-*.ckpt"), key=lambda p: p.stat().st_mtime, reverse=True)
    if bests:
        return bests[0]
    p = root / "last.ckpt"
    return p if p.exists() else None


def align_state_dict_keys(ckpt_sd: Dict, model_sd: Dict) -> Dict:
    """test.py:548-579: add / strip the "model." and "module." prefixes so a
    checkpoint of the core loads into the Lit wrapper and vice versa."""
    def frac(keys, p):
        ks = [k for k in keys if "." in k]
        return sum(k.startswith(p) for k in ks) / max(1, len(ks)) if ks else 0.0

    for p in ("model.", "module."):
        want, have = frac(list(model_sd), p) > 0.9, frac(list(ckpt_sd), p) > 0.9
        if want and not have:
            ckpt_sd = {(k if k.startswith(p) else p + k): v for k, v in ckpt_sd.items()}
        elif have and not want:
            ckpt_sd = {(k[len(p):] if k.startswith(p) else k): v for k, v in ckpt_sd.items()}
    return ckpt_sd


def materialize_lazy(model, depth, device):
    """FourierGate masks are created lazily at the first forward (models.py:1527-
    1533); create them at the run's depth so a checkpoint that holds
    them loads strictly."""
    for m in model.modules():
        if isinstance(m, M.FourierGate3D):
            m._ensure_mask(depth, device)


DETAIL_FIELDS = ["volume", "class", "dice", "sens", "spec"]
RANK_FIELDS = ["precision", "iou", "pr_auc", "roc_auc"]  # train.py:240-252, 313-323


def detail_fields():
    """Columns of test_details.csv; FAST_SIMPLE_METRICS=1 drops the ranking metrics."""
    return DETAIL_FIELDS + ([] if Hh.fast_simple_metrics() else RANK_FIELDS)


def predict_tiled(model, x, tiled, **kw):
    """Sliding-window inference of ``model`` with the ``tiled`` settings (--roi ...): on the
    forward-only plan where the module has one, through its forward otherwise."""
    if M.supports_predict(model):
        return model.predict_tiled(x, **tiled, **kw)
    return Hh.predict_tiled(model, x, **tiled, **kw)


def evaluate(model, dataset, K, device, tiled=None):
    """``tiled``: None, or the keywords of predict_tiled (roi, overlap, window_batch,
    mirror_axes): every variant is then evaluated on overlapping windows of ``roi`` whose
    logits are blended on the device; the ranking metrics take the blended scores as logits."""
    rows = []
    model.eval()
    rank = not Hh.fast_simple_metrics()
    # without the ranking metrics (they need the scores) the counts come from the head
    # itself: no logits are written or read back (models.py predict)
    fused = not rank and M.supports_predict(model)
    with torch.no_grad():
        for i in range(len(dataset)):
            x, y = dataset[i]
            x, y = x[None].to(device), y[None].to(device)
            if tiled is not None:
                out = predict_tiled(model, x, tiled, labels=y, ignore_index=255,
                                    return_scores=rank)
                logits = out[2] if rank else None
                dice, sens, spec, *_ = Hh.metrics_from_confusion(out[1].cpu().numpy(), K,
                                                                 int(y.numel()))
            elif fused:
                _mask, conf = model.predict(x, labels=y, ignore_index=255)
                dice, sens, spec, *_ = Hh.metrics_from_confusion(conf.cpu().numpy(), K,
                                                                 int(y.numel()))
            else:
                logits = model(x)
                dice, sens, spec, *_ = Hh.per_class_metrics_3d(logits, y, K, ignore_index=255)
            # each volume is a batch of one (train.py:773-798)
            rm = Hh.ranking_metrics(logits, y, K, per_sample=True) if rank else None
            for c in range(K):
                row = {"volume": i, "class": c, "dice": dice[c], "sens": sens[c], "spec": spec[c]}
                if rank:
                    row.update({k: rm[k][0][c] for k in RANK_FIELDS})
                rows.append(row)
    return rows


def write_case_overlays(model, dataset, n, out_dir, stem, device):
    """<out_dir>/<stem>_case<i>.png for the first ``n`` volumes: one forward each, then
    helpers.render_overlays."""
    paths = []
    model.eval()
    with torch.no_grad():
        for i in range(min(int(n), len(dataset))):
            x, y = dataset[i]
            x, y = x[None].to(device), y[None].to(device)
            strip = Hh.render_overlays(x, y, model(x), colors=getattr(C, "label_colors", None),
                                       max_items=1)
            paths.append(Hh.write_png(out_dir / f"{stem}_case{i}.png", strip[0]))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="analysis")
    ap.add_argument("--overlays", type=int, default=0, metavar="N",
                    help="draw the overlay figure of the first N test volumes per checkpoint")
    ap.add_argument("--roi", type=int, nargs=3, default=None, metavar=("D", "H", "W"),
                    help="sliding-window inference: run the network on overlapping windows of "
                         "this size and blend their logits with a Gaussian weight")
    ap.add_argument("--overlap", type=float, default=0.5, help="window overlap in [0, 1) (--roi)")
    ap.add_argument("--window-batch", type=int, default=1, help="windows per forward (--roi)")
    ap.add_argument("--mirror", default="", metavar="AXES",
                    help="test-time mirroring along these axes, e.g. 12 or 0,2 "
                         "(0 = D, 1 = H, 2 = W; --roi)")
    args = ap.parse_args(argv)
    tiled = None
    if args.roi is not None:
        tiled = {"roi": tuple(args.roi), "overlap": args.overlap,
                 "window_batch": args.window_batch,
                 "mirror_axes": tuple(sorted({int(c) for c in args.mirror if c.isdigit()}))}
    elif args.mirror or args.window_batch != 1 or args.overlap != 0.5:
        ap.error("--overlap, --window-batch and --mirror need --roi")
    S = Settings()
    device = torch.device("cuda", torch.cuda.current_device())
    out = pathlib.Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    summary = {}
    for name, builder, _dm, _base in C.selected_variants():
        for seed in S.seeds:
            ck = find_best_or_last_ckpt(S.ckpt_dir, name, seed)
            if ck is None:
                print(f"[test] {name} seed{seed}: no checkpoint under {S.ckpt_dir}")
                continue
            model = _build_lit(builder, S.in_ch).to(device)
            materialize_lazy(model, S.depth, device)
            sd = torch.load(ck, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd)
            model.load_state_dict(align_state_dict_keys(sd, model.state_dict()))
            K = int(model.hparams.num_classes)
            ds = SyntheticSPCCT(n=S.n_test, in_ch=S.in_ch, depth=S.depth, height=S.height,
                                width=S.width, num_classes=K, seed=seed + 20_000)
            rows = evaluate(model, ds, K, device, tiled)
            if args.overlays > 0:
                write_case_overlays(model, ds, args.overlays, out / "overlays",
                                    f"{name}_seed{seed}", device)
            det = ck.parent / "test_details.csv"
            with open(det, "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=detail_fields())
                w.writeheader()
                w.writerows(rows)
            for c in range(K):
                vals = [r["dice"] for r in rows if r["class"] == c and r["dice"] == r["dice"]]
                if vals:
                    summary.setdefault((name, c), []).append(statistics.fmean(vals))
            print(f"[test] {name} seed{seed}: {ck.name} -> {det}")
    with open(out / "per_class_summary.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["model", "class", "dice_mean", "dice_std", "n_seeds"])
        for (name, c), v in sorted(summary.items()):
            w.writerow([name, c, statistics.fmean(v), statistics.pstdev(v) if len(v) > 1 else 0.0,
                        len(v)])
    print(f"[test] wrote {out / 'per_class_summary.csv'}")


if __name__ == "__main__":
    main()
