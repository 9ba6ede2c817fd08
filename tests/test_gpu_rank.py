"""Ranking metrics on the GPU: spff_rank_auc (csrc/rank.hip), helpers.ranking_metrics and the
test-only block of BaseLitModel._shared_step against the fixtures the reference wrote with
scikit-learn (tests/golden/rank_*.npz) and against the numpy oracle.  Marked gpu.

Bounds.  Scores mode gets the fixture's own fp32 scores, so the tie structure is the
reference's and every count is an exact integer; what is left is the order of the fp64 sum,
at most n_groups * 2^-52 < 2e-11 for the largest segment here: 1e-9 absolute.  Logits mode
ranks the engine's own fp32 softmax, whose rounding can move a voxel between tie groups;
the yardstick is the reference's own sensitivity to that rounding, ``ref_d64`` (its metrics
from an fp64 softmax of the same logits), times the project's standing factor of 3
(FLIP_MULTIPLE of test_gpu_baseline_sizes.py), and never less than the scores-mode bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import _rank_oracle as RO
from innovative3D import _engine as E
from innovative3D import helpers as Hh
from innovative3D import models as M

pytestmark = pytest.mark.gpu

TOL = 1e-9
REF_MULTIPLE = 3.0
DEV = "cuda"


def _rows(scores_cl, labels, K, from_logits, per_sample):
    out = E.rank_auc(torch.from_numpy(np.array(scores_cl)).to(DEV),
                     torch.from_numpy(np.array(labels)).to(DEV), K, from_logits,
                     per_sample)
    return out.cpu().numpy()


def _fixture_rows(d, per_sample):
    """[rows, 2] (pr_auc, roc_auc) the reference logged, in spff_rank_auc's row order."""
    K, B = d["K"], d["B"]
    if per_sample:
        return np.array([[float(d[f"log_s{b}/test_{m}_class_{c}"]) for m in ("pr_auc", "roc_auc")]
                         for b in range(B) for c in range(K)])
    rows = [[float(d[f"log/test_{m}_class_{c}"]) for m in ("pr_auc", "roc_auc")] for c in range(K)]
    rows.append([float(d[f"log/test_{m}_micro"]) for m in ("pr_auc", "roc_auc")])
    return np.array(rows)


def _check(got, want, tol, what):
    """NaN positions equal, the rest within tol (per column when tol is a sequence);
    returns the largest differences per column."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    diff = np.where(np.isnan(want), 0.0, np.abs(got - want))
    worst = diff.reshape(-1, got.shape[-1]).max(0)
    print(f"{what}: max abs diff per column {worst}, bound {tol}")
    assert np.all(worst <= np.asarray(tol)), (what, worst, tol)
    return worst


def _counts(d, per_sample):
    ref = RO.rank_rows(d["scores_cl"], d["labels2"], d["K"], per_sample)
    return ref[:, 2:]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("name", RO.FIXTURES)
def test_scores_mode_matches_the_reference(name, per_sample):
    d = RO.load(name)
    got = _rows(d["scores_cl"], d["labels2"], d["K"], False, per_sample)
    assert np.array_equal(got[:, 2:], _counts(d, per_sample))  # n_pos, n_neg exact
    _check(got[:, :2], _fixture_rows(d, per_sample), TOL, f"{name} scores per_sample={per_sample}")


def _logit_bounds(d):
    return [max(REF_MULTIPLE * float(d[f"ref_d64/{m}"]), TOL) for m in ("pr_auc", "roc_auc")]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("name", RO.FIXTURES)
def test_logits_mode_within_the_references_own_sensitivity(name, per_sample):
    d = RO.load(name)
    got = _rows(d["logits_cl"], d["labels2"], d["K"], True, per_sample)
    assert np.array_equal(got[:, 2:], _counts(d, per_sample))
    _check(got[:, :2], _fixture_rows(d, per_sample), _logit_bounds(d),
           f"{name} logits per_sample={per_sample} (ref_d64 "
           f"{[float(d['ref_d64/' + m]) for m in ('pr_auc', 'roc_auc')]})")


def _synthetic(rounded):
    rng = np.random.default_rng(77)
    B, K, V = 1, 3, 70001  # odd: a ragged last tile, last wave and last key quad
    s = rng.random((B, V, K)).astype(np.float32)
    if rounded:
        s = (np.round(s * 8) / 8).astype(np.float32)  # nine tie groups
        s[0, ::1000, 1] = -0.0  # ranks with the +0.0 group
    y = rng.integers(0, K, size=(B, V)).astype(np.int64)
    y[rng.random((B, V)) < 0.05] = 255
    return s, y, K


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("rounded", [False, True])
def test_synthetic_multi_tile_against_the_oracle(rounded, per_sample):
    s, y, K = _synthetic(rounded)
    got = _rows(s, y, K, False, per_sample)
    want = RO.rank_rows(s, y, K, per_sample)
    assert np.array_equal(got[:, 2:], want[:, 2:])
    _check(got[:, :2], want[:, :2], TOL, f"synthetic rounded={rounded} per_sample={per_sample}")


def test_two_calls_give_the_same_bits():
    s, y, K = _synthetic(True)
    d = RO.load("rank_k13_multiblock")
    for sc, lab, k, fl in ((s, y, K, False), (d["logits_cl"], d["labels2"], d["K"], True)):
        for per_sample in (False, True):
            a = _rows(sc, lab, k, fl, per_sample)
            b = _rows(sc, lab, k, fl, per_sample)
            assert a.tobytes() == b.tobytes()


def test_single_class_has_a_nan_micro_row():
    rng = np.random.default_rng(5)
    s = rng.random((2, 100, 1)).astype(np.float32)
    y = rng.integers(0, 2, size=(2, 100)).astype(np.int64)
    got = _rows(s, y, 1, False, False)
    want = RO.rank_rows(s, y, 1, False)
    assert got.shape == (2, 4) and np.isnan(got[1, :2]).all() and np.array_equal(got[1, 2:], [0, 0])
    _check(got[:1, :2], want[:1, :2], TOL, "K = 1")


@pytest.mark.parametrize("per_sample", [False, True])
def test_many_classes_read_rows_from_memory(per_sample):
    """K = 40 is past the K up to which the key kernel stages rows in LDS, and its pooled tile
    is four units long; 4 500 voxels per sample give the per-sample segments two tiles."""
    rng = np.random.default_rng(9)
    B, V, K = 2, 4500, 40
    s = (np.round(rng.random((B, V, K)) * 64) / 64).astype(np.float32)
    y = rng.integers(0, K + 2, size=(B, V)).astype(np.int64)  # K, K + 1: negatives
    got = _rows(s, y, K, False, per_sample)
    want = RO.rank_rows(s, y, K, per_sample)
    assert np.array_equal(got[:, 2:], want[:, 2:])
    _check(got[:, :2], want[:, :2], TOL, f"K = 40 per_sample={per_sample}")
    # logits mode reads the same rows: softmax is monotone per row, so the counts agree
    lg = _rows(np.log(s + 1.0), y, K, True, per_sample)
    assert np.array_equal(lg[:, 2:], want[:, 2:]) and np.isfinite(lg[:, :2]).all()


class _Probe(M.BaseLitModel):
    """BaseLitModel whose network hands back the batch's "image": the stored logits."""

    def model(self, x):
        return x


def _logged(name, monkeypatch, fast, step="test_step"):
    d = RO.load(name)
    monkeypatch.setenv("FAST_SIMPLE_METRICS", "1" if fast else "0")
    lit = _Probe(num_classes=d["K"])
    lit.logged_metrics = {}
    batch = (torch.from_numpy(np.array(d["logits"])).to(DEV),
             torch.from_numpy(np.array(d["labels"])).to(DEV))
    with torch.no_grad():
        getattr(lit, step)(batch, 0)
    return d, {k: float(v) for k, v in lit.logged_metrics.items()}


@pytest.mark.parametrize("name", RO.FIXTURES)
def test_module_logs_the_references_test_keys(name, monkeypatch):
    d, full = _logged(name, monkeypatch, fast=False)
    K = d["K"]
    new = [k for k in full if any(k.startswith(f"test_{m}_") for m in RO.METRICS)]
    assert len(new) == 4 * K + 8
    assert sorted(full) == sorted(str(k) for k in d["keys"])  # exactly the reference's names
    for j, m in enumerate(RO.METRICS):
        tol = max(REF_MULTIPLE * float(d[f"ref_d64/{m}"]), TOL)
        keys = [f"test_{m}_class_{c}" for c in range(K)] + [f"test_{m}_macro", f"test_{m}_micro"]
        _check(np.array([[full[k]] for k in keys]), np.array([[float(d["log/" + k])] for k in keys]),
               tol, f"{name} module {m}")
    # FAST_SIMPLE_METRICS=1 drops the new keys and nothing else
    _d, fast = _logged(name, monkeypatch, fast=True)
    assert sorted(fast) == sorted(k for k in full if k not in new)
    for k, v in fast.items():
        assert v == full[k] or (np.isnan(v) and np.isnan(full[k])), k
    # the train prefix is untouched
    _d, train = _logged(name, monkeypatch, fast=False, step="training_step")
    assert sorted(train) == sorted(k.replace("test_", "train_", 1) for k in fast)


def test_ranking_metrics_per_sample_matches_the_single_sample_runs():
    d = RO.load("rank_ties_k5")
    K, B = d["K"], d["B"]
    rm = Hh.ranking_metrics(torch.from_numpy(np.array(d["logits"])).to(DEV),
                            torch.from_numpy(np.array(d["labels"])).to(DEV), K, per_sample=True)
    assert sorted(rm) == ["iou", "pr_auc", "precision", "roc_auc"]
    for m in RO.METRICS:
        tol = max(REF_MULTIPLE * float(d[f"ref_d64/{m}"]), TOL)
        want = np.array([[float(d[f"log_s{b}/test_{m}_class_{c}"]) for c in range(K)]
                         for b in range(B)])
        _check(np.array(rm[m]).reshape(-1, 1), want.reshape(-1, 1), tol, f"per-sample {m}")


def test_argument_checks():
    L = E.lib()
    s = torch.zeros(8, 4, device=DEV)
    y = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.zeros(5, 4, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for batch, vps, K in ((1, 8, 0), (1, 8, 129), (1, 0, 4), (0, 8, 4)):
        rc = L.spff_rank_auc(p(s), p(y), batch, vps, K, 0, 0, p(out), p(ws), None)
        assert rc == -1, (batch, vps, K, rc)  # SPFF_EINVAL
        assert b"spff_rank_auc" in L.spff_last_error()
    assert L.spff_rank_auc(None, p(y), 1, 8, 4, 0, 0, p(out), p(ws), None) == -1
    assert b"null" in L.spff_last_error()
    torch.cuda.synchronize()
    with pytest.raises(E.SpffError, match="num_classes"):
        E.rank_auc(torch.zeros(1, 2, 129, device=DEV), y[:2].reshape(1, 2), 129, False, False)
