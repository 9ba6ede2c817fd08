"""Every engine plan keeps the layout recorded in tests/golden/plan_layouts.json (taken from
the library before the six plans moved onto csrc/plan_base.h): flat parameter size, workspace
size, and the parameter (and buffer) table by name, shape, offset and count.  No GPU: creating
a plan only computes sizes."""
import json
import pathlib
import sys

import pytest

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_golden_plan_layouts as G  # noqa: E402

RECORD = json.loads((GOLDEN / "plan_layouts.json").read_text())


def test_record_covers_every_case():
    assert sorted(RECORD) == sorted(cid for cid, _cls, _kw in G.CASES)
    assert {cls for _cid, cls, _kw in G.CASES} == {"Plan", "UNet3DPlan", "SwinPlan", "UNETRPlan",
                                                   "R2UPlan", "RUPPPlan"}


@pytest.mark.parametrize("cid,cls,kw", G.CASES, ids=[c[0] for c in G.CASES])
def test_plan_layout_is_the_recorded_one(cid, cls, kw):
    from innovative3D import _engine as E
    assert G.layout(E, cls, kw) == RECORD[cid]
