"""The split-precision 3x3x3 weight gradient's tile walk and addressing: shapes at which the
incremental (b, h, w, d) walk, the per-column lane offsets and masks, the clamped
unconditional loads and the column staging can go wrong, against an fp64
torch.nn.grad.conv3d_weight.  Bound (as test_gpu_ops.py::test_conv3d_split_bf16): the error
is within 4x of the fp32 MFMA path's, plus 1e-7 of max|ref|.  Every case also runs twice and
must repeat bit for bit."""
import pytest
import torch

from innovative3D import _engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [
    # B, D, H, W, cin, cout, ksd
    (2, 1, 16, 16, 16, 32, 3),    # D = 1: every tile starts a column, all depth taps but one outside
    (2, 2, 24, 40, 16, 32, 3),    # D = 2: every second tile; roll-over across w, h and b
    (1, 5, 24, 40, 24, 48, 3),    # ragged H / W tiles, partial ci and co blocks, runs start mid-column
    (2, 3, 8, 16, 5, 32, 3),      # CI = 8 instantiation (ld 8), batch roll-over
    (1, 7, 16, 16, 40, 13, 3),    # Cout = 13 through the 16-wide output tile
    (2, 4, 16, 16, 32, 32, 1),    # ksd = 1: no plane ring
    (1, 130, 8, 16, 16, 32, 3),   # one column split over several workgroups
]


def _cl(t):  # [B,C,D,H,W] -> [B,D,H,W,C]
    return t.permute(0, 2, 3, 4, 1).contiguous()


_ref = {}


def _problem(case):
    """Inputs, the fp64 reference and the fp32 path's result of a case (computed once)."""
    if case not in _ref:
        B, D, H, W, cin, cout, ksd = case
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, cin, D, H, W, generator=g)
        dy = torch.randn(B, cout, D, H, W, generator=g)
        wshape = (cout, cin, ksd, 3, 3)
        dw64 = torch.nn.grad.conv3d_weight(x.double(), wshape, dy.double(),
                                           padding=(ksd // 2, 1, 1))
        ldx = (cin + 7) // 8 * 8
        xcl = torch.zeros(B, D, H, W, ldx)
        xcl[..., :cin] = _cl(x)
        # dy's channel stride is a multiple of 4 (the op's float4 loads): Cout = 13 is padded
        # to 16 zero-filled channels and goes through spff_conv3d_wgrad_ld, the others
        # through spff_conv3d_wgrad_ex (stride = Cout)
        lddy = (cout + 3) // 4 * 4
        dyg = torch.zeros(B, D, H, W, lddy)
        dyg[..., :cout] = _cl(dy)
        xcl, dyg = xcl.to(DEV), dyg.to(DEV)
        ws = torch.empty(E.lib().spff_conv3d_ws_bytes(B, D, H, W, cin, cout, ksd),
                         dtype=torch.uint8, device=DEV)
        _ref[case] = (xcl, ldx, dyg, ws, wshape, dw64, _wgrad(case, xcl, ldx, dyg, ws, wshape,
                                                             E.MATH_F32))
    return _ref[case]


def _wgrad(case, xcl, ldx, dyg, ws, wshape, math_id):
    B, D, H, W, cin, cout, ksd = case
    L, p, st = E.lib(), E._ptr, E._stream(torch.device(DEV))
    dw = torch.full(wshape, float("nan"), device=DEV)
    if dyg.shape[-1] == cout:
        rc = L.spff_conv3d_wgrad_ex(p(xcl), ldx, p(dyg), p(dw), B, D, H, W, cin, cout, ksd,
                                    math_id, p(ws), st)
    else:
        rc = L.spff_conv3d_wgrad_ld(p(xcl), ldx, p(dyg), dyg.shape[-1], p(dw), B, D, H, W, cin,
                                    cout, ksd, math_id, p(ws), st)
    E.check(rc, "wgrad")
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("math_mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("case", CASES)
def test_wgrad_tile_walk(case, math_mode):
    xcl, ldx, dyg, ws, wshape, dw64, dw32 = _problem(case)
    mth = E.MATH_NAMES[math_mode]
    dw = _wgrad(case, xcl, ldx, dyg, ws, wshape, mth)
    again = _wgrad(case, xcl, ldx, dyg, ws, wshape, mth)
    scale = float(dw64.abs().max())
    e32 = float((dw32.double() - dw64).abs().max())
    ex = float((dw.double() - dw64).abs().max())
    print(f"{math_mode} {case}: max err {ex / scale:.2e} of max|ref| (f32 path {e32 / scale:.2e})")
    assert torch.isfinite(dw).all()
    assert ex <= 4 * e32 + 1e-7 * scale, (ex, e32, scale)
    assert torch.equal(dw.view(torch.int32), again.view(torch.int32)), "not bitwise repeatable"
