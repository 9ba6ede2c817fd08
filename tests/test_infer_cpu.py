"""The forward-only layout (include/spff.h SPFF_MEM_INFER, memory="infer") on the host:
plan creation and sizes need no GPU.

The footprint bounds are derived, not measured: per input voxel at base 32 the
layout holds three level-0 buffers (3 x 128 B), the channel-last input padded to 8 channels
(32 B), the three pool outputs with their argmax bytes (32 + 16 + 8 B and 8 + 4 + 2 B = 70 B)
and the level-1 / level-2 skip buffers (64 + 32 B): 582 B; everything else is independent
of the volume or O(B C D)."""
import ctypes

import pytest

from innovative3D import _engine as E

SPFF_EINVAL = -1


def test_headline_footprint_per_voxel():
    V = 2 * 128 ** 3
    p = E.Plan(2, 5, 128, 128, 128, 13, memory="infer")
    lean = E.Plan(2, 5, 128, 128, 128, 13, memory="lean")
    print(f"infer {p.ws_bytes / V:.1f} B/voxel, lean {lean.ws_bytes / V:.1f} B/voxel")
    assert p.memory == "infer" and p.layout == "infer"
    assert p.ws_bytes / V <= 700, p.ws_bytes / V
    assert p.ws_bytes < 0.45 * lean.ws_bytes


def test_full_volume_512_footprint():
    p = E.Plan(1, 5, 512, 512, 512, 13, memory="infer")
    lean = E.Plan(1, 5, 512, 512, 512, 13, memory="lean")
    print(f"infer {p.ws_bytes / 2 ** 30:.1f} GiB, lean {lean.ws_bytes / 2 ** 30:.1f} GiB")
    assert p.ws_bytes <= 90 * 2 ** 30
    assert p.ws_bytes < 0.45 * lean.ws_bytes


def test_auto_never_selects_the_forward_only_layout():
    assert E.Plan(1, 5, 512, 512, 512, 13, memory="auto").layout == "lean"
    assert E.Plan(1, 5, 8, 32, 32, 13, memory="auto").layout == "full"


@pytest.mark.parametrize("kw", [
    dict(shard_world=2, shard_rank=0, shard_axis=0),   # depth-sharded
    dict(shard_world=2, shard_rank=1, shard_axis=1),   # height-sharded
    dict(spatial=True),
    dict(skip_gate=True),
], ids=["depth_sharded", "height_sharded", "spatial", "skip_gate"])
def test_forward_only_layout_rejects(kw):
    E.Plan(1, 5, 8, 32, 32, 13, base=8, memory="full", **kw)  # the full layout takes it
    with pytest.raises(E.SpffError, match=r"\(-1\)"):
        E.Plan(1, 5, 8, 32, 32, 13, base=8, memory="infer", **kw)


@pytest.mark.parametrize("flags", [(True, True, True, True), (False, False, False, False),
                                   (True, False, False, True), (False, True, True, False)])
@pytest.mark.parametrize("math", ["f32", "bf16x6", "bf16x3", "f16x3"])
def test_forward_only_plan_every_gate_combination(flags, math):
    ef, fg, se, sp = flags
    for shape, base in (((1, 5, 8, 36, 44), 8), ((2, 1, 5, 24, 40), 32)):
        kw = dict(base=base, efilm=ef, fgate=fg, se=se, specse=sp, math=math)
        p, full = (E.Plan(*shape, 13, memory=m, **kw) for m in ("infer", "full"))
        # (at these few voxels the weight images are most of it: both keep the batched ones)
        assert 0 < p.ws_bytes < full.ws_bytes
        assert p.params == full.params


def test_backward_on_forward_only_plan_is_einval_with_null_pointers():
    p = E.Plan(1, 5, 8, 32, 32, 13, base=8, memory="infer")
    rc = E.lib().spff_backward(p._h, None, None, None, None, None)
    assert rc == SPFF_EINVAL
    assert b"forward-only" in E.lib().spff_last_error()
    with pytest.raises(E.SpffError, match="forward-only"):
        p.backward(None, None)  # raised before any tensor is touched


def test_saved_tensor_of_forward_only_plan():
    """Only what the layout keeps has a name: the call fails before it forms a pointer."""
    p = E.Plan(1, 5, 8, 32, 32, 13, base=8, memory="infer")
    ws = (ctypes.c_char * 16)()
    ptr, nv, ch = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int()
    for name, want in ((b"enc1.y1", SPFF_EINVAL), (b"dec2.out", SPFF_EINVAL), (b"up1", SPFF_EINVAL),
                       (b"grad.out", SPFF_EINVAL), (b"x_cl", 0), (b"pool2.idx", 0),
                       (b"dec1.y2", 0), (b"bott.al2", 0)):
        rc = E.lib().spff_saved_tensor(p._h, ws, name, ctypes.byref(ptr), ctypes.byref(nv),
                                       ctypes.byref(ch))
        assert rc == want, name


def test_predict_argument_checks_need_no_device():
    """conf exactly when labels; logits where the streaming head does not cover the plan."""
    L = E.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    p8 = E.Plan(1, 5, 4, 16, 16, 6, base=8, memory="infer")
    assert not p8.streams_head()
    assert L.spff_predict(p8._h, one, one, one, None, None, 0, 0, None, one, None) == SPFF_EINVAL
    assert b"logits must be given" in L.spff_last_error()
    p32 = E.Plan(1, 5, 4, 16, 16, 13, base=32, memory="infer")
    assert p32.streams_head()
    assert L.spff_predict(p32._h, one, one, one, None, one, 1, 255, None, one, None) == SPFF_EINVAL
    assert L.spff_predict(p32._h, one, one, None, None, None, 0, 0, None, one, None) == SPFF_EINVAL


def test_environment_default_is_never_forward_only(monkeypatch):
    monkeypatch.setenv("SPFF_MEMORY", "infer")
    with pytest.raises(E.SpffError):
        E.default_memory()
