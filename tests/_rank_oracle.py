"""Numpy definition of the ranking metrics of csrc/rank.hip: what the reference gets from
scikit-learn's ``auc(*precision_recall_curve(y, s)[1::-1])`` and ``roc_auc_score(y, s)``
(models.py:530-533, 560-563), written out.  fp64, a stable sort on the fp32 bit pattern,
no scikit-learn import.  tests/test_rank_cpu.py pins it to the values the reference wrote
into tests/golden/rank_*.npz.

Group the voxels by exactly equal fp32 score, groups in descending score order; tp_g, fp_g
the cumulative positives / negatives after group g (tp_0 = fp_0 = 0), P and N the totals:
    roc_auc = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1}) / (2 P N)
    pr_auc  = sum_g (r_g - r_{g-1}) (p_g + p_{g-1}) / 2,  p_g = tp_g / (tp_g + fp_g),
              r_g = tp_g / P, p_0 = 1, r_0 = 0
Both are NaN when P == 0 or N == 0.
"""
import functools
import pathlib

import numpy as np

FIXTURES = ("rank_small_k4", "rank_ties_k5", "rank_k13_multiblock")
METRICS = ("pr_auc", "roc_auc", "iou", "precision")


@functools.lru_cache(maxsize=None)
def load(name):
    """A rank_*.npz fixture as a dict (loaded once per session, never modified), plus
    "K", "B", "scores_cl" / "logits_cl" [B, V, K] and "labels2" [B, V]."""
    with np.load(pathlib.Path(__file__).resolve().parent / "golden" / f"{name}.npz") as z:
        d = {k: z[k] for k in z.files}
    B, K = d["logits"].shape[:2]
    d["B"], d["K"] = int(B), int(K)
    d["scores_cl"] = np.ascontiguousarray(np.moveaxis(d["scores"], 1, -1)).reshape(B, -1, K)
    d["logits_cl"] = np.ascontiguousarray(np.moveaxis(d["logits"], 1, -1)).reshape(B, -1, K)
    d["labels2"] = d["labels"].reshape(B, -1)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def logged(d, metric, tag=""):
    """The fixture's K class values of ``metric`` ("pr_auc", ...) of the batch run (tag "")
    or of sample b's run (tag "_s<b>"), and its macro and micro values."""
    K = d["K"]
    cls = np.array([float(d[f"log{tag}/test_{metric}_class_{c}"]) for c in range(K)])
    return (cls, float(d[f"log{tag}/test_{metric}_macro"]),
            float(d[f"log{tag}/test_{metric}_micro"]))


def pr_roc(y, s):
    """(pr_auc, roc_auc, n_pos, n_neg) of binary labels y and scores s (finite, >= 0)."""
    y = np.asarray(y).astype(np.int64).ravel()
    s = np.asarray(s, dtype=np.float32).ravel()
    n = y.size
    P = int(y.sum())
    N = n - P
    if P == 0 or N == 0:
        return float("nan"), float("nan"), P, N
    key = (s + np.float32(0.0)).view(np.uint32).astype(np.int64)  # (-0.0 + 0.0 = +0.0)
    order = np.argsort(-key, kind="stable")
    k, yy = key[order], y[order]
    ends = np.r_[np.nonzero(np.diff(k))[0], n - 1]
    tp = np.cumsum(yy)[ends]
    fp = ends + 1 - tp
    tp0, fp0 = np.r_[0, tp], np.r_[0, fp]
    num = int(np.sum((fp0[1:] - fp0[:-1]) * (tp0[1:] + tp0[:-1])))  # exact integers
    roc = num / (2.0 * P * N)
    prec = tp / (tp + fp).astype(np.float64)
    rec = tp / float(P)
    p0, r0 = np.r_[1.0, prec], np.r_[0.0, rec]
    pr = float(np.sum((r0[1:] - r0[:-1]) * (p0[1:] + p0[:-1]) / 2))
    return pr, roc, P, N


def rank_rows(scores_cl, labels, K, per_sample):
    """The rows spff_rank_auc writes: scores_cl [B, V, K] (channel-last), labels [B, V].
    Pooled: K class rows and the micro row (classes 1..K-1 concatenated; NaN for K < 2);
    per sample: B * K rows in (b, c) order.  float64 [rows, 4]."""
    scores_cl = np.asarray(scores_cl, dtype=np.float32)
    B = scores_cl.shape[0]
    s = scores_cl.reshape(B, -1, K)
    y = np.asarray(labels).reshape(B, -1)
    rows = []
    if per_sample:
        for b in range(B):
            for c in range(K):
                rows.append(pr_roc(y[b] == c, s[b, :, c]))
    else:
        for c in range(K):
            rows.append(pr_roc(y == c, s[:, :, c]))
        if K > 1:
            rows.append(pr_roc(np.concatenate([(y == c).ravel() for c in range(1, K)]),
                               np.concatenate([s[:, :, c].ravel() for c in range(1, K)])))
        else:
            rows.append((float("nan"), float("nan"), 0, 0))
    return np.array(rows, dtype=np.float64)


def confusion(logits_cl, labels, K):
    """conf[pred, label] of the argmax (first maximum wins) without an ignore mask:
    [K, K + 1], column K = labels outside [0, K)."""
    lg = np.asarray(logits_cl).reshape(-1, K)
    y = np.asarray(labels).ravel()
    pred = lg.argmax(1)
    col = np.where((y >= 0) & (y < K), y, K)
    conf = np.zeros((K, K + 1), dtype=np.int64)
    np.add.at(conf, (pred, col), 1)
    return conf
