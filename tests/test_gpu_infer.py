"""Inference on the engine: the forward-only layout (memory="infer", SPFF_MEM_INFER) and
the fused class-mask head (spff_predict).  Marked gpu.

Same kernels on the same operands, placed elsewhere: a forward-only plan's logits are
BITWISE the full layout's, and the mask / confusion counts the head forms from the logits
it holds in registers are exactly torch.argmax / spff_confusion of those logits.

Shapes: the smallest extent with three pools on the GEMM head (base 8); ragged H, W (the
_cat resize and its raw up-conv output); base 32 with HW % 256 == 0 (the streaming head's
shared-coefficient arm, fused a1 / out); the registry layout with HW = 960 (the general
loader arm and a partial last tile)."""
import csv
import functools
import io
import sys

import numpy as np
import pytest
import torch

from _compare import check_logits
from _golden import load
from _spff_checks import load_core, synth_core

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (shape, base, K)
CASES = {
    "pools_b8": ((2, 5, 4, 16, 16), 8, 6),
    "ragged_b8": ((1, 5, 8, 36, 44), 8, 6),
    "stream_hw256": ((1, 5, 8, 32, 32), 32, 13),
    "registry_hw960": ((2, 1, 5, 24, 40), 32, 13),
}
BITWISE = [(n, "f16x3") for n in CASES] + [("stream_hw256", "f32"), ("stream_hw256", "bf16x6")]


def _model(case, math_mode, memory):
    """tests/test_gpu_memory.py::_model at this case's shape, base and K"""
    shape, base, K = CASES[case]
    core = synth_core(K, base, shape[1], shape[2], 13, 0.25)[0].to(DEV)
    core.math, core.memory = math_mode, memory
    return core


def _inputs(case, seed):
    """x, and labels with 5 % ignored voxels and a few outside [0, K) (value K + 3)"""
    from innovative3D.synthetic import synthetic_batch
    shape, _base, K = CASES[case]
    x, y = synthetic_batch(*shape, num_classes=K, ignore_frac=0.05, seed=seed)
    y.view(-1)[::97] = K + 3
    return x.to(DEV), y.to(DEV)


@functools.lru_cache(maxsize=None)
def _full_logits(case, math_mode):
    """The full layout's no-grad logits [B, K, D, H, W] for inputs 3 and 4 (computed once,
    never written to)"""
    full = _model(case, math_mode, "full")
    with torch.no_grad():
        out = tuple(full(_inputs(case, s)[0]).clone() for s in (3, 4))
    return out + (full._infer_plan.ws_bytes,)


@pytest.mark.parametrize("case,math_mode", BITWISE)
def test_forward_only_logits_bitwise(case, math_mode):
    ref_a, ref_b, full_ws = _full_logits(case, math_mode)
    infer = _model(case, math_mode, "infer")
    xa, xb = _inputs(case, 3)[0], _inputs(case, 4)[0]
    with torch.no_grad():
        # two inputs, then the first again: nothing of a forward survives into the next
        for x, ref in ((xa, ref_a), (xb, ref_b), (xa, ref_a)):
            assert torch.equal(infer(x), ref)
    assert infer._infer_plan.layout == "infer"
    assert infer._infer_plan.ws_bytes < full_ws


@pytest.mark.parametrize("case", list(CASES))
def test_predict_mask_and_counts(case):
    from innovative3D import _engine as E
    K = CASES[case][2]
    ref = _full_logits(case, "f16x3")[0]
    ref_cl = ref.permute(0, 2, 3, 4, 1).contiguous()
    x, y = _inputs(case, 3)
    core = _model(case, "f16x3", None)
    want_mask = torch.argmax(ref, 1).to(torch.uint8)
    for ign in (255, None):
        want_conf = E.confusion(ref_cl, y, K, ign)
        mask, conf, logits = core.predict(x, labels=y, ignore_index=ign, return_logits=True)
        assert mask.dtype == torch.uint8 and mask.shape == y.shape
        assert torch.equal(mask, want_mask)
        assert conf.dtype == torch.int64 and torch.equal(conf, want_conf)
        assert torch.equal(logits, ref)
        # without the logits (never written where the head streams)
        mask2, conf2 = core.predict(x, labels=y, ignore_index=ign)
        assert torch.equal(mask2, want_mask) and torch.equal(conf2, want_conf)
    assert int(want_conf[:, K].sum()) > 0  # the out-of-range labels reached column K
    assert torch.equal(core.predict(x), want_mask)
    assert core._infer_plan.layout == "infer"


@pytest.mark.parametrize("memory", ["full", "lean"])
@pytest.mark.parametrize("case", ["pools_b8", "registry_hw960"])
def test_predict_on_plans_that_keep_a_backward(case, memory):
    """spff_predict runs on every memory mode (lean: dec1's output is stored, so the fused
    head reads plain rows, not y2 through the activation)."""
    from innovative3D import _engine as E
    K = CASES[case][2]
    x, y = _inputs(case, 3)
    core = _model(case, "f16x3", None)
    plan = core._engine_plan(x, "infer", memory=memory)
    assert plan.layout == memory
    flat = core._ensure_flat(plan, core._engine_params(plan), x.device)
    ref_cl = plan.forward(x, flat).clone()  # this plan's own spff_forward
    mask, conf, logits_cl = plan.predict(x, flat, y, 255, want_logits=True)
    assert torch.equal(logits_cl, ref_cl)
    assert torch.equal(mask, torch.argmax(ref_cl, 4).to(torch.uint8))
    assert torch.equal(conf, E.confusion(ref_cl, y, K, 255))
    mask2, conf2, none = plan.predict(x, flat, y, 255)
    assert none is None and torch.equal(mask2, mask) and torch.equal(conf2, conf)


@pytest.mark.parametrize("case", ["pools_b8", "registry_hw960"])
def test_predict_ties_take_the_first_class(case):
    """Zero head weight and bias: every voxel's K logits tie, the mask is all zero."""
    K = CASES[case][2]
    core = _model(case, "f16x3", None)
    with torch.no_grad():
        core.out.weight.zero_()
        core.out.bias.zero_()
    x, y = _inputs(case, 3)
    mask, conf, logits = core.predict(x, labels=y, ignore_index=255, return_logits=True)
    assert not logits.any() and not mask.any()
    valid = y != 255
    assert int(conf[0].sum()) == int(valid.sum()) and int(conf[1:].sum()) == 0
    assert int(conf[0, K]) == int((valid & (y >= K)).sum())


@pytest.mark.parametrize("name", ["fx1_registry_k13", "fx3b_fgate_odd_b2", "fx4_ragged_hw",
                                  "fx5_k40_base24"])
def test_forward_only_matches_reference_fixture(name):
    """tests/test_gpu_parity.py's forward bar on a forward-only plan: logits within 1e-3 of
    the reference's, identical argmax outside near-ties (fx5: K = 40, the row-argmax pass)."""
    d = load(name)
    K = d["meta"]["K"]
    core = load_core(d)
    core.math, core.memory = "f16x3", "infer"
    x = torch.from_numpy(d["x"]).to(DEV)
    y = torch.from_numpy(d["labels"]).to(DEV)
    with torch.no_grad():
        lg = core(x).cpu().numpy()
    assert core._infer_plan.layout == "infer"
    check_logits(name, lg, d["logits"])
    mask, conf = core.predict(x, labels=y, ignore_index=255)
    assert np.array_equal(mask.cpu().numpy().astype(np.int64), lg.argmax(1))
    assert int(conf.sum()) == int((y != 255).sum())


def test_forward_only_guards():
    from innovative3D import _engine as E
    case = "pools_b8"
    core = _model(case, "f16x3", "infer")
    x = _inputs(case, 3)[0]
    with pytest.raises(E.SpffError, match="forward-only"):
        core(x)  # a forward that needs a gradient
    with torch.no_grad():
        logits = core(x)
    plan = core._infer_plan
    flat = core._flat
    with pytest.raises(E.SpffError, match="forward-only"):
        plan.backward(torch.zeros_like(logits.permute(0, 2, 3, 4, 1)), flat)
    with pytest.raises(E.SpffError, match="does not keep"):
        plan.saved("enc1.y1")
    assert plan.saved("pool1").shape[1] == CASES[case][1]
    # leaving .memory unset trains as before
    core.memory = None
    core(x).sum().backward()
    assert core.out.weight.grad is not None


def test_evaluate_rows_from_the_fused_head(monkeypatch):
    """test.py evaluate with FAST_SIMPLE_METRICS=1 takes the counts from predict: the rows
    (and test_details.csv's bytes) of the logits path, model(x) + per_class_metrics_3d."""
    import innovative3D.helpers as Hh
    import innovative3D.models as M
    from innovative3D.synthetic import SyntheticSPCCT
    monkeypatch.setenv("FAST_SIMPLE_METRICS", "1")
    sys.modules.pop("test", None)
    import test as TT
    K = 13
    torch.manual_seed(5)
    model = M.LitSPCT_EFiLM_FourierGate(num_classes=K, base=32).to(DEV)
    TT.materialize_lazy(model, 5, DEV)
    assert M.supports_predict(model)
    ds = SyntheticSPCCT(n=2, in_ch=1, depth=5, height=16, width=16, num_classes=K, seed=11)
    rows = TT.evaluate(model, ds, K, torch.device(DEV))
    assert model.model._infer_plan.layout == "infer"
    old = []
    model.eval()
    with torch.no_grad():
        for i in range(len(ds)):
            x, y = ds[i]
            x, y = x[None].to(DEV), y[None].to(DEV)
            dice, sens, spec, *_ = Hh.per_class_metrics_3d(model(x), y, K, ignore_index=255)
            old += [{"volume": i, "class": c, "dice": dice[c], "sens": sens[c], "spec": spec[c]}
                    for c in range(K)]

    def text(rr):
        f = io.StringIO()
        w = csv.DictWriter(f, fieldnames=TT.detail_fields())
        w.writeheader()
        w.writerows(rr)
        return f.getvalue()
    assert TT.detail_fields() == TT.DETAIL_FIELDS
    assert text(rows) == text(old)
