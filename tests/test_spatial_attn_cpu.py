"""CPU-only checks of the op-level spatial attention entry points: the argument checks
return before any device call, and the Python wrappers refuse host tensors."""
import ctypes

import pytest
import torch

from innovative3D import _engine as E


def test_ws_bytes_and_argument_checks():
    L = E.lib()
    # dt [V] + dm [V][2] + one 294-float row per 16 x 16 tile + the next reduction level
    V, tiles = 2 * 5 * 24 * 40, 2 * 5 * 2 * 3
    ws = int(L.spff_spatial_attn_ws_bytes(2, 5, 24, 40, 32))
    assert 4 * (3 * V + 294 * (tiles + 1)) <= ws <= 4 * (3 * V + 294 * (tiles + 1)) + 4 * 256
    assert ws == int(L.spff_spatial_attn_ws_bytes(2, 5, 24, 40, 256))  # no term in C
    for bad in ((1, 1, 1, 1, 12), (1, 1, 1, 1, 0), (0, 1, 1, 1, 8), (1, 1, 1, -1, 8)):
        assert int(L.spff_spatial_attn_ws_bytes(*bad)) == 0
        assert b"multiple of 8" in L.spff_last_error()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    assert L.spff_spatial_attn_fwd(one, one, 1, 1, 1, 1, 12, one, one, one, one, None,
                                   None) == -1
    assert L.spff_spatial_attn_fwd(None, one, 1, 1, 1, 1, 8, one, one, one, one, None,
                                   None) == -1
    assert b"null" in L.spff_last_error()
    assert L.spff_spatial_attn_fwd(ctypes.c_void_p(4), one, 1, 1, 1, 1, 8, one, one, one, one,
                                   None, None) == -1
    assert b"aligned" in L.spff_last_error()
    assert L.spff_spatial_attn_bwd(one, one, one, one, one, one, 1, 1, 1, 1, 8, one, one, None,
                                   None) == -1


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    x = torch.zeros(1, 1, 2, 2, 8)
    w = torch.zeros(1, 2, 3, 7, 7)
    with pytest.raises(E.SpffError, match="ROCm"):
        E.spatial_attn_fwd(x, w)
    with pytest.raises(E.SpffError, match="ROCm"):
        E.spatial_attn_bwd(x, x, w, x[..., 0], x[..., :2], x[..., 0].int())
