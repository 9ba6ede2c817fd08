"""The comparison rules themselves (tests/_compare.py, and the SPFF bar of
tests/_spff_checks.py) on synthetic arrays of a few dozen elements.  CPU-only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _compare import check_grads_rows, check_logits, grad_errors, kink_hooks, near_tie_mask
from _spff_checks import check_grads, grad_scales


def _ref64():
    """one tensor of 24 entries, max|g64| = 1 (the default scale), entry 1 exactly 0"""
    g = np.random.default_rng(0).uniform(-0.5, 0.5, 24)
    g[0], g[1] = 1.0, 0.0
    return {"w": g}


def _off(ref64, delta, i=1):
    g = ref64["w"].copy()
    g[i] += delta
    return {"w": g}


def _check(grads, ref64, ref32, **kw):
    scale = kw.pop("scale", None)
    check_grads_rows(grad_errors(grads, ref64, ref32, scale=scale), **kw)


# ------------------------------------------------------------------ gradients --
@pytest.mark.parametrize("value", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_one_nan_or_inf_in_a_gradient_fails(value, as_tensor):
    ref64 = _ref64()
    _check(_off(ref64, 0.0), ref64, _off(ref64, 1e-7))  # the clean gradient passes
    grads = _off(ref64, value, i=7)
    if as_tensor:
        grads = {"w": torch.from_numpy(grads["w"]).float()}
    with pytest.raises(AssertionError, match="w: gpu"):
        _check(grads, ref64, _off(ref64, 1e-7))
    with pytest.raises(AssertionError, match="w: gpu"):
        _check(grads, ref64, None)


def test_missing_gradient_fails():
    ref64 = _ref64()
    with pytest.raises(AssertionError, match="w"):
        grad_errors({"w": None}, ref64, None)


def test_nan_in_the_fp32_oracle_fails():
    ref64 = _ref64()
    with pytest.raises(AssertionError, match="w: gpu"):
        _check(_off(ref64, 0.0), ref64, _off(ref64, math.nan, i=3))


@pytest.mark.parametrize("floor,factor,e32", [(1e-3, 8, 2.5e-4), (1e-3, 16, 1e-3), (5e-3, 64, 1e-4),
                                              (1e-3, 8, 1e-5)])
def test_the_bar_itself_passes_and_the_next_float_fails(floor, factor, e32):
    ref64 = _ref64()
    ref32 = _off(ref64, e32)
    (_a, got32, _k), = grad_errors(ref64, ref64, ref32)
    assert got32 == e32
    tol = max(floor, factor * e32)
    (e_gpu, _b, _k), = grad_errors(_off(ref64, tol), ref64, ref32)
    assert e_gpu == tol
    _check(_off(ref64, tol), ref64, ref32, floor=floor, factor=factor)
    with pytest.raises(AssertionError, match="w: gpu"):
        _check(_off(ref64, np.nextafter(tol, 1.0)), ref64, ref32, floor=floor, factor=factor)


def test_floor_alone_without_an_fp32_run():
    ref64 = _ref64()
    assert grad_errors(ref64, ref64, None) == [(0.0, 0.0, "w")]
    _check(_off(ref64, 1e-3), ref64, None, factor=1e9)
    with pytest.raises(AssertionError, match="w: gpu"):
        _check(_off(ref64, np.nextafter(1e-3, 1.0)), ref64, None, factor=1e9)


def test_per_key_scale_is_honoured():
    ref64 = _ref64()
    ref64["v"] = ref64["w"].copy()
    grads = {"w": _off(ref64, 0.5)["w"], "v": ref64["v"]}
    rows = grad_errors(grads, ref64, None, scale={"w": 1000.0})
    assert rows == [(0.5 / 1000.0, 0.0, "w"), (0.0, 0.0, "v")]  # "v": the default, max|g64|
    check_grads_rows(rows)
    with pytest.raises(AssertionError, match="w: gpu 5.00e-01"):
        _check(grads, ref64, None)


def test_worst_rows_are_printed_nan_first(capsys):
    rows = [(1e-5, 0.0, "a"), (math.nan, 0.0, "b"), (3e-4, 0.0, "c"), (2e-4, 0.0, "d")]
    with pytest.raises(AssertionError, match="^b: gpu nan vs fp32-oracle 0.00e\\+00$"):
        check_grads_rows(rows, top=3, width=4)
    assert capsys.readouterr().out.splitlines() == [
        "  b    gpu nan  fp32-oracle 0.00e+00", "  c    gpu 3.00e-04  fp32-oracle 0.00e+00",
        "  d    gpu 2.00e-04  fp32-oracle 0.00e+00"]


# --------------------------------------------------------------------- logits --
E = 2.0 ** -12  # how far the flip cases move a logit: exactly representable sums


def _logits(nvox_tied=0, gap=None):
    """ref [1, 3, 1, 3, 4]: class 1 leads by 1 everywhere, but by ``gap`` over class 0 at the
    first ``nvox_tied`` voxels; lg moves those two logits by E towards each other there."""
    ref = np.zeros((1, 3, 1, 3, 4))
    ref[0, 0], ref[0, 2] = -1.0, -2.0
    lg = ref.copy()
    for v in range(nvox_tied):
        ref[0, 0, 0, v // 4, v % 4] = -gap
        lg[0, 0, 0, v // 4, v % 4] = -gap + E
        lg[0, 1, 0, v // 4, v % 4] = -E
    return lg, ref


def test_error_at_the_bound_passes_and_just_over_fails():
    lg, ref = _logits()
    lg[0, 1, 0, 2, 3] = 1e-3
    assert check_logits("t", lg, ref)[:2] == (1e-3, 0)
    lg[0, 1, 0, 2, 3] = np.nextafter(1e-3, 1.0)
    with pytest.raises(AssertionError, match="max.dlogit"):
        check_logits("t", lg, ref)
    check_logits("t", lg, ref, max_err=2e-3)


def test_flip_at_a_near_tie_passes_and_at_a_wider_gap_fails():
    # gap just under 2 E: class 0 overtakes class 1, at a near-tie of the reference
    lg, ref = _logits(1, np.nextafter(2 * E, 0.0))
    err, nf, flips = check_logits("t", torch.from_numpy(lg), ref)
    assert (err, nf) == (E, 1) and flips[0, 0, 0, 0] and flips.sum() == 1
    assert near_tie_mask(ref, 2 * err).sum() == 1
    # gap = 2 E = 2 err: the moved logits tie, argmax takes class 0 -- the same flip, but the
    # reference's gap is not below 2 err
    lg, ref = _logits(1, 2 * E)
    assert lg[0, 0, 0, 0, 0] == lg[0, 1, 0, 0, 0]
    with pytest.raises(AssertionError, match="1 of 1 argmax flips outside near-ties"):
        check_logits("t", lg, ref)


def test_flip_cap():
    lg, ref = _logits(9, np.nextafter(2 * E, 0.0))
    assert check_logits("t", lg, ref)[1] == 9
    assert check_logits("t", lg, ref, max_flips=9)[1] == 9
    with pytest.raises(AssertionError, match="9 argmax flips, at most 8"):
        check_logits("t", lg, ref, max_flips=8)


def test_nan_logits_fail():
    lg, ref = _logits()
    lg[0, 2, 0, 1, 1] = math.nan
    with pytest.raises(AssertionError, match="max.dlogit"):
        check_logits("t", lg, ref)
    with pytest.raises(AssertionError, match="max.dlogit"):
        check_logits("t", torch.from_numpy(lg).float(), ref.astype(np.float32))


# ----------------------------------------------------------------- kink hooks --
def _decisions():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 2, 2, 4, 4, generator=g)
    masks = {"b.out": torch.randn(1, 2, 2, 4, 4, generator=g) > 0, "a.a1": x > 0}
    pooled, idx = F.max_pool3d(x, 2, return_indices=True)
    return x, pooled, masks, {"pool1": idx}


def test_kink_hooks_relu_and_pool():
    x, pooled, masks, pidx = _decisions()
    hooks, _digest = kink_hooks(masks, pidx)
    for dt in (torch.float32, torch.float64):
        r = hooks["relu"]("a.a1", x.to(dt))
        assert r.dtype == dt and torch.equal(r, torch.relu(x).to(dt))
        r = hooks["relu"]("b.out", x.to(dt))
        assert r.dtype == dt and torch.equal(r, torch.where(masks["b.out"], x, 0 * x).to(dt))
    assert torch.equal(hooks["pool"]("pool1", x), pooled)
    v = torch.arange(x.numel(), dtype=torch.float64).view(x.shape)  # v's entries: flat indices
    got = hooks["pool"]("pool1", v)
    assert got.shape == pooled.shape
    per_channel = v - v.flatten(2)[:, :, :1].view(1, 2, 1, 1, 1)
    assert torch.equal(hooks["pool"]("pool1", per_channel).long(), pidx["pool1"])


def test_kink_hooks_digest_follows_every_decision():
    _x, _p, masks, pidx = _decisions()
    digest = kink_hooks(masks, pidx)[1]
    assert len(digest) == 64
    same = kink_hooks({k: v.clone() for k, v in reversed(list(masks.items()))},
                      {k: v.clone() for k, v in pidx.items()})[1]
    assert same == digest
    m2 = {k: v.clone() for k, v in masks.items()}
    m2["b.out"][0, 1, 1, 3, 3] ^= True
    assert kink_hooks(m2, pidx)[1] != digest
    p2 = {"pool1": pidx["pool1"].clone()}
    p2["pool1"][0, 1, 0, 1, 1] ^= 1
    assert kink_hooks(masks, p2)[1] != digest


# ------------------------------------------------------------- the SPFF bar --
def _spff_case(mag):
    pre = "enc1.fgate."
    ref64 = {pre + "mag_scale": np.array([0.1]), pre + "freq_mask": np.array([0.1, -0.2, 0.3, 0.4]),
             "w": np.array([1.0, 0.0, -0.5])}
    absb = {k: np.abs(v) for k, v in ref64.items()}
    absb[pre + "mag_scale"] = np.array([0.2])  # two samples' terms, partly cancelling
    st = {pre + "mag_scale": np.array([mag], np.float32),
          pre + "freq_mask": np.array([1.0, 2.0, -1.0, 0.5], np.float32)}
    return ref64, absb, st


def test_mag_scale_scale_is_the_larger_candidate():
    pre = "enc1.fgate."
    # sum_k |mask_k g_mask_k| = 0.1 + 0.4 + 0.3 + 0.2 = 1
    ref64, absb, st = _spff_case(mag=-0.5)
    s = grad_scales(ref64, absb, st)
    assert s["w"] == 1.0 and s[pre + "freq_mask"] == 0.4
    assert math.isclose(s[pre + "mag_scale"], 1.0 / 0.5, rel_tol=1e-12)
    grads = {k: v.copy() for k, v in ref64.items()}
    grads[pre + "mag_scale"] += 1.5e-3  # 7.5e-4 of 2, 7.5e-3 of 0.2
    check_grads(grads, ref64, None, absb, st, "f32")
    ref64, absb, st = _spff_case(mag=50.0)  # the terms' sum 0.02 is below sum_b |g_b| = 0.2
    assert grad_scales(ref64, absb, st)[pre + "mag_scale"] == 0.2
    with pytest.raises(AssertionError, match="mag_scale: gpu 7.50e-03"):
        check_grads(grads, ref64, None, absb, st, "f32")


def test_bf16x3_takes_its_own_floor_and_factor():
    ref64, absb, st = _spff_case(mag=-0.5)
    grads = {k: v.copy() for k, v in ref64.items()}
    grads["w"][1] = 4e-3
    check_grads(grads, ref64, None, absb, st, "bf16x3")  # floor 5e-3
    for mth in ("f32", "bf16x6", "f16x3"):
        with pytest.raises(AssertionError, match="w: gpu 4.00e-03"):
            check_grads(grads, ref64, None, absb, st, mth)
    ref32 = {k: v.copy() for k, v in ref64.items()}
    ref32["w"][1] = 1e-4
    grads["w"][1] = 6e-3  # within 64 x 1e-4, above 5e-3 and above 8 x 1e-4
    check_grads(grads, ref64, ref32, absb, st, "bf16x3")
    grads["w"][1] = np.nextafter(64 * 1e-4, 1.0)
    with pytest.raises(AssertionError, match="w: gpu 6.40e-03"):
        check_grads(grads, ref64, ref32, absb, st, "bf16x3")
    grads["w"][1] = math.nan
    with pytest.raises(AssertionError, match="w: gpu nan"):
        check_grads(grads, ref64, ref32, absb, st, "bf16x3")
