"""Ranking metrics (csrc/rank.hip, helpers.ranking_metrics), the part that needs no GPU:
the numpy oracle reproduces what the reference and scikit-learn wrote into the fixtures,
the IoU / precision algebra of helpers reproduces them from a numpy confusion matrix, the
workspace stays inside its documented bound, and there is no CPU fallback."""
import numpy as np
import pytest
import torch

import _rank_oracle as RO
from innovative3D import _engine as E
from innovative3D import helpers as Hh


def _same(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    m = ~np.isnan(want)
    assert np.all(np.abs(got[m] - want[m]) <= tol), (what, np.abs(got[m] - want[m]).max())


@pytest.mark.parametrize("name", RO.FIXTURES)
def test_oracle_reproduces_the_reference(name):
    d = RO.load(name)
    K, B = d["K"], d["B"]
    assert str(d["sklearn_version"]) and len(d["keys"]) >= 4 * K + 8
    rows = RO.rank_rows(d["scores_cl"], d["labels2"], K, per_sample=False)
    for j, metric in enumerate(("pr_auc", "roc_auc")):
        cls, _macro, micro = RO.logged(d, metric)
        _same(rows[:K, j], cls, 1e-12, (name, metric))
        _same(rows[K, j], micro, 1e-12, (name, metric, "micro"))
    per = RO.rank_rows(d["scores_cl"], d["labels2"], K, per_sample=True).reshape(B, K, 4)
    for b in range(B):
        for j, metric in enumerate(("pr_auc", "roc_auc")):
            cls, _macro, micro = RO.logged(d, metric, f"_s{b}")
            _same(per[b, :, j], cls, 1e-12, (name, metric, b))
            one = RO.rank_rows(d["scores_cl"][b:b + 1], d["labels2"][b:b + 1], K, False)
            _same(one[K, j], micro, 1e-12, (name, metric, b, "micro"))


def test_fixtures_hold_the_cases_they_are_for():
    d = RO.load("rank_ties_k5")
    iou, _ma, _mi = RO.logged(d, "iou")
    prec, _ma, _mi = RO.logged(d, "precision")
    pr, pr_macro, _mi = RO.logged(d, "pr_auc")
    assert iou[3] == 0.0 and prec[3] == 0.0 and np.isnan(pr[3])   # predicted, never labelled
    assert np.isnan(iou[4]) and np.isnan(prec[4]) and np.isnan(pr[4])  # absent from both
    assert np.isfinite(pr_macro)  # the macro mean skips the NaN classes
    s = d["scores_cl"]
    assert (s == 1.0).sum() > 50 and ((s > 0) & (s < 1e-30)).sum() > 50  # big tie groups
    assert (RO.load("rank_small_k4")["labels"] == 255).any()
    k13 = RO.load("rank_k13_multiblock")
    assert k13["labels2"].size == 5760 and k13["K"] == 13


@pytest.mark.parametrize("name", RO.FIXTURES)
def test_iou_precision_algebra_reproduces_the_reference(name):
    d = RO.load(name)
    K, B = d["K"], d["B"]
    runs = [("", slice(0, B))] + [(f"_s{b}", slice(b, b + 1)) for b in range(B)]
    for tag, sl in runs:
        conf = RO.confusion(d["logits_cl"][sl], d["labels2"][sl], K)
        iou, prec, iou_ma, prec_ma, iou_mi, prec_mi = Hh.iou_precision_from_confusion(conf, K)
        for got, metric in (((iou, iou_ma, iou_mi), "iou"), ((prec, prec_ma, prec_mi), "precision")):
            cls, macro, micro = RO.logged(d, metric, tag)
            _same(got[0], cls, 1e-12, (name, tag, metric))
            _same(got[1], macro, 1e-12, (name, tag, metric, "macro"))
            _same(got[2], micro, 1e-12, (name, tag, metric, "micro"))


def test_iou_precision_unguarded_micro_and_single_class():
    # nothing labelled or predicted in the foreground: sklearn's zero_division gives 0
    conf = np.zeros((3, 4), dtype=np.int64)
    conf[0, 0] = 10
    iou, prec, iou_ma, prec_ma, iou_mi, prec_mi = Hh.iou_precision_from_confusion(conf, 3)
    assert iou[0] == 1.0 and np.isnan(iou[1]) and np.isnan(prec[2])
    assert np.isnan(iou_ma) and np.isnan(prec_ma) and iou_mi == 0.0 and prec_mi == 0.0
    one = Hh.iou_precision_from_confusion(np.array([[5, 2]]), 1)
    assert one[0] == [5 / 7] and one[2] == 5 / 7 and np.isnan(one[4]) and np.isnan(one[5])


def test_no_cpu_fallback():
    lg = torch.zeros(1, 3, 2, 4, 4)
    y = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    with pytest.raises(E.SpffError):
        Hh.ranking_metrics(lg, y, 3)
    with pytest.raises(E.SpffError):
        E.rank_auc(lg.permute(0, 2, 3, 4, 1), y, 3, True, False)
    assert "ranking_metrics" in Hh.__all__


def test_workspace_bound():
    """spff_rank_auc_ws_bytes <= 16 K B V + 1 MiB: two key buffers for the class segments
    and the micro segment plus scan state, also for tiny and for many-class shapes."""
    L = E.lib()
    for per_sample in (0, 1):
        for B in (1, 2, 7, 4096):
            for V in (1, 3, 192, 4097, 70001, 5 * 512 * 512):
                for K in (1, 2, 13, 16, 17, 128):
                    if B * V * K > 1 << 31:
                        continue
                    n = int(L.spff_rank_auc_ws_bytes(B, V, K, per_sample))
                    keys = 8 * B * V * (K if per_sample or K < 2 else 2 * K - 1)
                    assert keys < n <= 16 * K * B * V + (1 << 20), (per_sample, B, V, K, n)
    for bad in ((0, 10, 3), (1, 0, 3), (1, 10, 0), (1, 10, 129)):
        assert L.spff_rank_auc_ws_bytes(*bad, 0) == 0
