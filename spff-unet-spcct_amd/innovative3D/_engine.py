"""ctypes binding of libspff_hip.so (include/spff.h) + the torch glue around it.

There is deliberately no CPU / PyTorch fallback: if the HIP library is
missing or the tensors are not on a ROCm device, every entry point raises.
"""
from __future__ import annotations

import collections
import ctypes
import inspect
import os
import pathlib
import threading
import weakref
from typing import Dict, List, Optional, Tuple

import torch

_LIB_PATH = pathlib.Path(__file__).resolve().parent / "_lib" / "libspff_hip.so"
_lib = None
_lib_lock = threading.Lock()


class SpffError(RuntimeError):
    pass


class SpffCollError(SpffError):
    """A shard-group collective (spff_coll callback: halo exchange or all-reduce) failed,
    e.g. a peer rank died or timed out; the engine returned SPFF_ECOLL."""


SPFF_ECOLL = -4


class spff_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("num_classes", ctypes.c_int),
        ("base", ctypes.c_int), ("ksd", ctypes.c_int), ("use_efilm", ctypes.c_int),
        ("use_fgate", ctypes.c_int), ("use_se", ctypes.c_int), ("use_specse", ctypes.c_int),
        ("math", ctypes.c_int), ("shard_world", ctypes.c_int), ("shard_rank", ctypes.c_int),
        ("memory_mode", ctypes.c_int), ("shard_axis", ctypes.c_int),
        ("efilm_hidden", ctypes.c_int), ("efilm_pe_dims", ctypes.c_int),
        ("fgate_learn_phase", ctypes.c_int), ("use_spatial", ctypes.c_int),
        ("use_skip_gate", ctypes.c_int),
    ]


class spff_unet3d_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("target_depth", ctypes.c_int),
        ("num_classes", ctypes.c_int), ("base", ctypes.c_int), ("math", ctypes.c_int),
        ("reserved", ctypes.c_int * 7),
    ]


class spff_r2u_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("num_classes", ctypes.c_int),
        ("base", ctypes.c_int), ("t", ctypes.c_int), ("math", ctypes.c_int),
        ("reserved", ctypes.c_int * 7),
    ]


class spff_rupp_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("num_classes", ctypes.c_int),
        ("base", ctypes.c_int), ("math", ctypes.c_int), ("reserved", ctypes.c_int * 8),
    ]


class spff_swin_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("num_classes", ctypes.c_int),
        ("feature_size", ctypes.c_int), ("window", ctypes.c_int), ("heads", ctypes.c_int * 4),
        ("mlp_ratio", ctypes.c_float), ("math", ctypes.c_int), ("reserved", ctypes.c_int * 6),
    ]


class spff_unetr_cfg(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int), ("in_ch", ctypes.c_int), ("depth", ctypes.c_int),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("img", ctypes.c_int * 3),
        ("num_classes", ctypes.c_int), ("feature_size", ctypes.c_int), ("hidden", ctypes.c_int),
        ("mlp_dim", ctypes.c_int), ("heads", ctypes.c_int), ("math", ctypes.c_int),
        ("reserved", ctypes.c_int * 6),
    ]


# spff_coll (include/spff.h): the shard group's collectives, called back by the engine
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_int, ctypes.c_void_p)
HALO_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                           ctypes.c_int, ctypes.c_void_p)


class spff_coll(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("allreduce", ALLREDUCE_FN), ("halo", HALO_FN)]


# spff_grad_ready_fn (include/spff.h): dparams[off, off + n) final during spff_backward
GRAD_READY_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                 ctypes.c_void_p)


# saved-activation layout (include/spff.h SPFF_MEM_*)
# ("infer": the forward-only layout, SPFF_MEM_INFER -- asked for by name, never a default)
MEMORY_MODES = {"auto": 0, "full": 1, "lean": 2, "infer": 3}
_DEFAULT_MEMORY_MODES = ("auto", "full", "lean")


def default_memory() -> str:
    """Saved-activation layout for new plans: $SPFF_MEMORY, else "auto" (lean from 2^26
    voxels per plan)."""
    m = os.environ.get("SPFF_MEMORY", "auto")
    if m not in _DEFAULT_MEMORY_MODES:
        raise SpffError(f"SPFF_MEMORY={m!r}: expected one of {sorted(_DEFAULT_MEMORY_MODES)}")
    return m


# conv arithmetic (include/spff.h SPFF_MATH_*)
MATH_F32, MATH_BF16X6, MATH_BF16X3, MATH_F16X3 = 0, 1, 2, 3
MATH_NAMES = {"f32": MATH_F32, "bf16x6": MATH_BF16X6, "bf16x3": MATH_BF16X3,
              "f16x3": MATH_F16X3}


def default_math() -> str:
    """Conv arithmetic for new plans: $SPFF_MATH, else "f16x3" (scaled fp16 planes, measured
    as close to fp64 as the fp32 MFMA path)."""
    m = os.environ.get("SPFF_MATH", "f16x3")
    if m not in MATH_NAMES:
        raise SpffError(f"SPFF_MATH={m!r}: expected one of {sorted(MATH_NAMES)}")
    return m


_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_S = ctypes.c_size_t

_ENTRIES = ("create", "destroy", "num_params", "param_info", "param_floats", "workspace_bytes",
            "forward", "backward", "saved_tensor")


def _entry_names(prefix: str) -> Dict[str, str]:
    """The symbols of the nine entry points every plan has (include/spff.h)."""
    return {k: f"{prefix}_{k}" for k in _ENTRIES}


# the main plan's symbols predate the per-plan prefixes
_MAIN_NAMES = {**_entry_names("spff"), "create": "spff_plan_create",
               "destroy": "spff_plan_destroy"}


def _plan_sigs(names: Dict[str, str], cfg) -> Dict[str, tuple]:
    sigs = {
        "create": (_I, [ctypes.POINTER(cfg), ctypes.POINTER(_P)]),
        "destroy": (None, [_P]),
        "num_params": (_I, [_P]),
        "param_info": (_I, [_P, _I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_I),
                            ctypes.POINTER(_L), ctypes.POINTER(_L), ctypes.POINTER(_L)]),
        "param_floats": (_L, [_P]),
        "workspace_bytes": (_S, [_P]),
        "forward": (_I, [_P, _P, _P, _P, _P, _P]),
        "backward": (_I, [_P, _P, _P, _P, _P, _P]),
        "saved_tensor": (_I, [_P, _P, ctypes.c_char_p, ctypes.POINTER(_P), ctypes.POINTER(_L),
                              ctypes.POINTER(_I)]),
    }
    return {names[k]: sigs[k] for k in _ENTRIES}


_SIGS = {
    **_plan_sigs(_MAIN_NAMES, spff_cfg),
    **_plan_sigs(_entry_names("spff_unet3d"), spff_unet3d_cfg),
    **_plan_sigs(_entry_names("spff_r2u"), spff_r2u_cfg),
    **_plan_sigs(_entry_names("spff_rupp"), spff_rupp_cfg),
    **_plan_sigs(_entry_names("spff_swin"), spff_swin_cfg),
    **_plan_sigs(_entry_names("spff_unetr"), spff_unetr_cfg),
    "spff_plan_set_coll": (_I, [_P, ctypes.POINTER(spff_coll)]),
    "spff_plan_set_grad_hook": (_I, [_P, GRAD_READY_FN, _P]),
    "spff_last_error": (ctypes.c_char_p, []),
    "spff_predict": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "spff_debug_set": (_I, [_P, _I, _I]),
    "spff_prof_enable": (_I, [_P, _I]),
    "spff_prof_collect": (_I, [_P, ctypes.POINTER(ctypes.c_double), _I]),
    "spff_upconv_ws_bytes": (ctypes.c_size_t, [_I, _I, _I, _I, _I, _I]),
    "spff_upconv_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_upconv_dgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_upconv_wgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_spatial_attn_ws_bytes": (_S, [_I, _I, _I, _I, _I]),
    "spff_spatial_attn_fwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "spff_spatial_attn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "spff_unet3d_set_sync_bn": (_I, [_P, _P, _I]),
    "spff_conv_prof_enable": (_I, [_I]),
    "spff_conv_prof_collect": (_I, [ctypes.POINTER(ctypes.c_double), _I]),
    "spff_loss_ws_bytes": (_S, [_L, _I]),
    "spff_loss": (_I, [_P, _P, _L, _I, _I, ctypes.c_double, _P, _P, _P, _P, _P, _P]),
    "spff_confusion": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "spff_count_valid": (_I, [_P, _L, _I, _P, _P]),
    "spff_rank_auc_ws_bytes": (_S, [_I, _L, _I, _I]),
    "spff_rank_auc": (_I, [_P, _P, _I, _L, _I, _I, _I, _P, _P, _P]),
    "spff_pred_views_ws_bytes": (_S, [_I, _I, _I, _I, _I]),
    "spff_pred_views": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "spff_input_views": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "spff_overlay_rgb": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "spff_tile_gather": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P]),
    "spff_tile_accumulate": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "spff_tile_finalize": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, ctypes.c_float, _P, _P, _P, _I,
                                _I, _P, _P]),
    "spff_scale": (_I, [_P, _L, _P, _P]),
    "spff_conv3d_ws_bytes": (_S, [_I, _I, _I, _I, _I, _I, _I]),
    "spff_conv3d_fwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_dgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_adam_step": (_I, [_P, _P, _P, _P, _L, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                            ctypes.c_double, ctypes.c_double, _I, _L, _P]),
    "spff_conv3d_fwd_ex": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_dgrad_ex": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_wgrad_ex": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_wgrad_ld": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_wgrad": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    # 3DUNet baseline variant (BASELINE config 3)
    "spff_unet3d_num_buffers": (_I, [_P]),
    "spff_unet3d_buffer_info": (_I, [_P, _I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_L),
                                     ctypes.POINTER(_L)]),
    "spff_unet3d_buffer_floats": (_L, [_P]),
    # (replaces the standard forward above: buffers and training between params and logits)
    "spff_unet3d_forward": (_I, [_P, _P, _P, _P, _I, _P, _P, _P]),
    # R2UNet3D variant
    "spff_r2u_dice_loss_ws_bytes": (_S, [_I, _I]),
    "spff_r2u_dice_loss": (_I, [_P, _P, _I, _L, _I, _I, _I, _P, _P, _P, _P]),
    # ResUNet++ variant
    "spff_rupp_loss_ws_bytes": (_S, [_I, _I]),
    "spff_rupp_loss": (_I, [_P, _P, _I, _L, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double,
                            _P, _P, _P, _P]),
    # the voxel-weighted 3DUNet loss and the nnU-Net Dice + CE loss
    "spff_unet3d_loss_ws_bytes": (_S, [_I, _I]),
    "spff_unet3d_loss": (_I, [_P, _P, _I, _L, _I, _I, _I, _P, _P, _I, ctypes.c_double,
                              ctypes.c_double, _P, _P, _P, _P]),
    "spff_nnunet_loss_ws_bytes": (_S, [_I, _I]),
    "spff_nnunet_loss": (_I, [_P, _P, _I, _L, _I, _I, _I, _I, ctypes.c_double, ctypes.c_double,
                              _P, _P, _P, _P]),
    "spff_conv3d_dil_ws_bytes": (_S, [_I, _I]),
    "spff_conv3d_dil_fwd": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_dil_dgrad": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "spff_conv3d_dil_wgrad": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    # SwinUNETR variant (BASELINE config 5)
    "spff_swin_loss_ws_bytes": (_S, [_I, _I]),
    # UNETR variant
    "spff_vit_attn_ws_bytes": (_S, [_I, _I, _I]),
    "spff_vit_attn_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "spff_vit_attn_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "spff_resize3d_fwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "spff_resize3d_bwd": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    # data path
    "spff_rasterize_ellipses": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "spff_resize_bilinear_aa": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P]),
    "spff_grid_aug_ws_bytes": (_S, [_I]),
    "spff_grid_aug": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, ctypes.c_uint64, _P, _P, _P, _P]),
    "spff_swin_loss": (_I, [_P, _P, _I, _L, _I, _I, _I, ctypes.c_double, _P, _P, _P, _P]),
    "spff_loss_ex": (_I, [_P, _P, _L, _I, _I, ctypes.c_double, _P, _P, _I, _P, _P, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)


def lib_path() -> pathlib.Path:
    return pathlib.Path(os.environ.get("SPFF_LIB", str(_LIB_PATH)))


def lib():
    """Load libspff_hip.so (raises if it is missing -- no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            p = lib_path()
            if not p.exists():
                raise SpffError(
                    f"libspff_hip.so not found at {p}; build it with "
                    f"`python spff-unet-spcct_amd/build_ext.py` (hipcc, gfx950)")
            L = ctypes.CDLL(str(p))
            for name, (res, args) in _SIGS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().spff_last_error()
        raise SpffError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_device(t: torch.Tensor, what: str):
    if not (t.is_cuda and torch.version.hip is not None):
        raise SpffError(f"{what}: the SPFF engine runs only on a ROCm (HIP) device; got a tensor "
                        f"on {t.device}. There is no CPU fallback.")


class _PlanBase:
    """What every engine plan shares (DESIGN "Plan scaffolding"): the handle, the parameter
    table, the workspace and forward / backward / saved on the plan's nine entry points.

    A plan class sets PREFIX (its C symbols are ``{PREFIX}_create`` ...), CFG (the ctypes
    struct), NAME (used in messages) and ``_fill_cfg``; its ``__init__`` keeps the keyword
    signature and passes what is its own through.  The workspace holds the saved
    activations of the most recent forward until the matching backward (``generation``
    guards against interleaving)."""

    PREFIX = CFG = NAME = None
    ENTRY_NAMES: Optional[Dict[str, str]] = None  # only where the symbols are irregular

    def __init__(self, batch, in_ch, depth, height, width, num_classes, device, math, **own):
        math = math or default_math()
        if math not in MATH_NAMES:
            raise SpffError(f"math={math!r}: expected one of {sorted(MATH_NAMES)}")
        cfg = self.CFG()
        cfg.batch, cfg.in_ch, cfg.depth, cfg.height, cfg.width = batch, in_ch, depth, height, width
        cfg.num_classes, cfg.math = num_classes, MATH_NAMES[math]
        self.cfg, self.math, self.device = cfg, math, device
        self._fill_cfg(cfg, **own)
        h = ctypes.c_void_p()
        self._check(self._fn("create")(ctypes.byref(cfg), ctypes.byref(h)), self._sym("create"))
        self._h = h
        self.params: List[Tuple[str, Tuple[int, ...], int, int]] = []
        info = self._fn("param_info")
        for i in range(self._fn("num_params")(h)):
            name, nd = ctypes.c_char_p(), ctypes.c_int()
            shape, off, n = (ctypes.c_int64 * 5)(), ctypes.c_int64(), ctypes.c_int64()
            self._check(info(h, i, ctypes.byref(name), ctypes.byref(nd), shape, ctypes.byref(off),
                             ctypes.byref(n)), self._sym("param_info"))
            self.params.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)),
                                off.value, n.value))
        self.nfloats = int(self._fn("param_floats")(h))
        self.ws_bytes = int(self._fn("workspace_bytes")(h))
        self._ws: Optional[torch.Tensor] = None
        self.generation = 0

    def _fill_cfg(self, cfg) -> None:
        """Set the cfg fields beyond batch .. num_classes and math."""

    @classmethod
    def _sym(cls, entry: str) -> str:
        return cls.ENTRY_NAMES[entry] if cls.ENTRY_NAMES else f"{cls.PREFIX}_{entry}"

    def _fn(self, entry: str):
        return getattr(lib(), self._sym(entry))

    _check = staticmethod(check)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and _lib is not None:
                getattr(_lib, self._sym("destroy"))(self._h)
        except Exception:
            pass

    def workspace(self, device) -> torch.Tensor:
        if self._ws is None or self._ws.device != device:
            self._ws = _alloc_workspace(self, device)
        return self._ws

    def forward(self, x: torch.Tensor, flat: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B,Cin,D,H,W] fp32 -> logits channel-last [B,D,H,W,K]."""
        return self._forward(x, flat, out)

    def _forward(self, x, flat, out, *extra):
        """``extra``: the plan's own arguments between params and logits"""
        c = self.cfg
        require_device(x, f"{self.NAME} forward")
        if tuple(x.shape) != (c.batch, c.in_ch, c.depth, c.height, c.width):
            raise SpffError(f"input shape {tuple(x.shape)} does not match plan")
        if x.dtype != torch.float32:
            raise SpffError("the engine computes in fp32; got " + str(x.dtype))
        x = x.contiguous()
        if out is None:
            out = torch.empty((c.batch, c.depth, c.height, c.width, c.num_classes),
                              dtype=torch.float32, device=x.device)
        ws = self.workspace(x.device)
        self.generation += 1
        self._check(self._fn("forward")(self._h, _ptr(x), _ptr(flat), *extra, _ptr(out), _ptr(ws),
                                        _stream(x.device)), self._sym("forward"))
        return out

    def backward(self, dlogits_cl: torch.Tensor, flat: torch.Tensor,
                 dflat: Optional[torch.Tensor] = None, grad_hook=None) -> torch.Tensor:
        """``grad_hook`` (GradBucketer protocol): the whole gradient is reported as ready
        once the backward is enqueued (no per-block hook)."""
        dlogits_cl = dlogits_cl.contiguous()
        if dflat is None:
            dflat = torch.empty(self.nfloats, dtype=torch.float32, device=dlogits_cl.device)
        ws = self.workspace(dlogits_cl.device)
        self._check(self._fn("backward")(self._h, _ptr(dlogits_cl), _ptr(flat), _ptr(dflat),
                                         _ptr(ws), _stream(dlogits_cl.device)),
                    self._sym("backward"))
        _whole_buffer_hook(grad_hook, dflat)
        return dflat

    def _saved_view(self, name: str) -> Tuple[torch.Tensor, int, int]:
        """(bytes of the workspace from the saved tensor on, rows, channels)"""
        ws = self._ws
        if ws is None:
            raise SpffError("no forward has run")
        ptr, nv, ch = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int()
        self._check(self._fn("saved_tensor")(self._h, _ptr(ws), name.encode(), ctypes.byref(ptr),
                                             ctypes.byref(nv), ctypes.byref(ch)),
                    self._sym("saved_tensor"))
        return ws[ptr.value - ws.data_ptr():], nv.value, ch.value

    def saved(self, name: str) -> torch.Tensor:
        """Copy of a saved intermediate as a channel-last fp32 [V, C] tensor (debug/tests)."""
        b, nv, ch = self._saved_view(name)
        return b[:4 * nv * ch].view(torch.float32).view(nv, ch).clone()


def _whole_buffer_hook(grad_hook, dflat: torch.Tensor) -> None:
    if grad_hook is None:
        return
    grad_hook.begin(dflat)
    grad_hook.ready(0, int(dflat.numel()))
    grad_hook.finish()


class Plan(_PlanBase):
    """One plan of the main SPFF engine (shape + flags) and its device workspace; beyond
    _PlanBase: sharding, the memory mode, per-block gradient hooks, profiling and debug keys."""

    CFG, NAME, ENTRY_NAMES = spff_cfg, "SPFF", _MAIN_NAMES

    def __init__(self, batch, in_ch, depth, height, width, num_classes, base=32, ksd=3,
                 efilm=True, fgate=True, se=True, specse=True, device=None, math=None,
                 shard_world=1, shard_rank=0, memory=None, shard_axis=0, efilm_hidden=32,
                 efilm_pe_dims=16, fgate_learn_phase=False, spatial=False, skip_gate=False):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math,
                         base=base, ksd=ksd, efilm=efilm, fgate=fgate, se=se, specse=specse,
                         shard=(int(shard_world), int(shard_rank), int(shard_axis)),
                         memory=memory, efilm_hidden=efilm_hidden, efilm_pe_dims=efilm_pe_dims,
                         fgate_learn_phase=fgate_learn_phase, spatial=spatial,
                         skip_gate=skip_gate)
        self.key = (batch, in_ch, depth, height, width, num_classes, base, ksd, bool(efilm),
                    bool(fgate), bool(se), bool(specse), self.math, self.shard, self.memory,
                    int(efilm_hidden), int(efilm_pe_dims), bool(fgate_learn_phase),
                    bool(spatial), bool(skip_gate))

    def _fill_cfg(self, cfg, base, ksd, efilm, fgate, se, specse, shard, memory, efilm_hidden,
                  efilm_pe_dims, fgate_learn_phase, spatial=False, skip_gate=False):
        memory = default_memory() if memory is None else memory
        if memory not in MEMORY_MODES:
            raise SpffError(f"memory={memory!r}: expected one of {sorted(MEMORY_MODES)}")
        cfg.memory_mode = MEMORY_MODES[memory]
        self.memory = memory
        # UNet3D_SpectralCore(use_spatial, use_skip_gate): unsharded, never the lean layout
        cfg.use_spatial, cfg.use_skip_gate = int(bool(spatial)), int(bool(skip_gate))
        attn = bool(spatial) or bool(skip_gate)
        # the layout the engine resolves (engine.hip build_plan: lean from 2^26 voxels on auto)
        voxels = cfg.batch * cfg.depth * cfg.height * cfg.width
        self.layout = ("infer" if memory == "infer" else "lean" if memory == "lean" or
                       (memory == "auto" and voxels >= 1 << 26 and not attn) else "full")
        # axis 0 = SPFF_SHARD_DEPTH (BASELINE config 4), 1 = SPFF_SHARD_HEIGHT (registry layout)
        cfg.shard_world, cfg.shard_rank, cfg.shard_axis = self.shard = shard
        cfg.base, cfg.ksd = base, ksd
        cfg.use_efilm, cfg.use_fgate, cfg.use_se, cfg.use_specse = (int(bool(efilm)), int(bool(fgate)),
                                                                    int(bool(se)), int(bool(specse)))
        # EnergyFiLM3D(hidden, pe_dims) / FourierGate3D(learn_phase) of the blocks
        cfg.efilm_hidden, cfg.efilm_pe_dims = int(efilm_hidden), int(efilm_pe_dims)
        cfg.fgate_learn_phase = int(bool(fgate_learn_phase))

    def set_coll(self, impl) -> None:
        """Attach a depth-sharding collective implementation: an object with
        ``allreduce(t)`` (in-place sum of a device tensor over the group) and
        ``halo(slab, slice, d_local)`` (``slab`` = the [d_local + 2] x slice view
        whose first / last slices receive the neighbours' boundary slices), e.g.
        innovative3D.sharded.TorchDepthColl.  The engine calls them in stream
        order with pointers into this plan's workspace."""
        def view(ptr, n, dtype):
            ws = self._ws
            off = ptr - ws.data_ptr()
            esz = 8 if dtype == torch.float64 else 4
            if off < 0 or off % esz or off + n * esz > ws.numel():
                raise SpffError("collective buffer outside the plan workspace")
            return ws[off:off + n * esz].view(dtype)

        def _timed(kind, nbytes, stream, dev, fn):
            """fn(); with coll_timing on, bracketed by HIP events on the stream the engine
            handed the callback (where the collective's work is issued)"""
            if not self.coll_timing:
                return fn()
            st = (torch.cuda.ExternalStream(stream, device=dev) if stream
                  else torch.cuda.current_stream(dev))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            fn()
            b.record(st)
            self._coll_ev.append((kind, nbytes, a, b))

        def _allreduce(ctx, buf, n, dt, stream):
            try:
                t = view(buf, n, torch.float64 if dt == 1 else torch.float32)
                nb = t.numel() * t.element_size()
                cur = torch.cuda.current_stream(t.device)
                if stream and stream != cur.cuda_stream:
                    # issue the all-reduce on the stream the engine handed over (where
                    # its timing events are recorded and the buffer is ordered), as
                    # _halo does
                    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=t.device)):
                        _timed("allreduce", nb, stream, t.device, lambda: impl.allreduce(t))
                else:
                    _timed("allreduce", nb, stream, t.device, lambda: impl.allreduce(t))
                return 0
            except Exception as e:  # noqa: BLE001 -- reported through the engine status
                self.coll_error = e
                return 1

        def _halo(ctx, interior, sl, d_local, stream):
            try:
                slab = view(interior - 4 * sl, (d_local + 2) * sl, torch.float32)
                cur = torch.cuda.current_stream(slab.device)
                # 2 slices sent (and 2 received) per rank at most
                nb = 2 * 4 * int(sl)
                if stream and stream != cur.cuda_stream:
                    # the engine's side stream (halo exchange overlapping the interior
                    # depth tiles of the next convolution): issue the exchange there
                    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=slab.device)):
                        _timed("halo", nb, stream, slab.device,
                               lambda: impl.halo(slab, int(sl), int(d_local)))
                else:
                    _timed("halo", nb, stream, slab.device,
                           lambda: impl.halo(slab, int(sl), int(d_local)))
                return 0
            except Exception as e:  # noqa: BLE001
                self.coll_error = e
                return 1
        self.coll_timing = getattr(self, "coll_timing", False)
        self._coll_ev = []
        self._coll_fns = (ALLREDUCE_FN(_allreduce), HALO_FN(_halo))  # keep alive
        self._coll = spff_coll(None, self._coll_fns[0], self._coll_fns[1])
        self.coll_impl = impl
        self.coll_error = None
        check(lib().spff_plan_set_coll(self._h, ctypes.byref(self._coll)), "spff_plan_set_coll")

    def coll_collect(self) -> Dict[str, Dict[str, float]]:
        """{kind: {calls, ms, bytes}} of the shard-group collective callbacks since the
        last collect (coll_timing on: HIP events around each callback's work on its
        stream; a halo on the side stream overlaps the interior conv tiles, so its time
        is the exchange's duration, not the step time it costs).  Syncs on the events."""
        out: Dict[str, Dict[str, float]] = {}
        for kind, nb, a, b in getattr(self, "_coll_ev", []):
            b.synchronize()
            r = out.setdefault(kind, {"calls": 0, "ms": 0.0, "bytes": 0.0})
            r["calls"] += 1
            r["ms"] += a.elapsed_time(b)
            r["bytes"] += nb
        self._coll_ev = []
        return out

    def forward(self, x: torch.Tensor, flat: torch.Tensor, out: Optional[torch.Tensor] = None):
        self.coll_error = None
        return self._forward(x, flat, out)

    def _check(self, rc: int, what: str) -> None:
        """check(), raising SpffCollError chained to the callback's own exception when a
        shard-group collective failed (SPFF_ECOLL)"""
        if rc == SPFF_ECOLL:
            msg = lib().spff_last_error()
            err = getattr(self, "coll_error", None)
            raise SpffCollError(f"{what} failed ({rc}): {msg.decode() if msg else ''}"
                                + (f" -- {err!r}" if err is not None else "")) from err
        check(rc, what)

    def backward(self, dlogits_cl: torch.Tensor, flat: torch.Tensor,
                 dflat: Optional[torch.Tensor] = None, grad_hook=None) -> torch.Tensor:
        """``grad_hook``: an object with begin(dflat), ready(off, n) and finish()
        (innovative3D.distributed.GradBucketer); ready() is called while the
        backward is being enqueued, as each parameter group's gradient becomes
        final, and finish() after it."""
        if self.layout == "infer":  # before any device call
            raise SpffError("forward-only plan (memory='infer'): nothing is kept for a backward")
        dlogits_cl = dlogits_cl.contiguous()
        if dflat is None:
            dflat = torch.empty(self.nfloats, dtype=torch.float32, device=dlogits_cl.device)
        ws = self.workspace(dlogits_cl.device)
        L = lib()
        self.coll_error = None
        if grad_hook is None:
            self._check(L.spff_backward(self._h, _ptr(dlogits_cl), _ptr(flat), _ptr(dflat),
                                        _ptr(ws), _stream(dlogits_cl.device)), "spff_backward")
            return dflat
        covered = [0]
        err = []

        dev = dlogits_cl.device
        main_stream = torch.cuda.current_stream(dev).cuda_stream

        def _ready(_ctx, off, n, stream):
            try:
                covered[0] += int(n)
                if stream and stream != main_stream:
                    # the engine's weight-gradient stream (those floats are final in its
                    # order): the bucket's all-reduce is issued there
                    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                        grad_hook.ready(int(off), int(n))
                else:
                    grad_hook.ready(int(off), int(n))
                return 0
            except Exception as e:  # noqa: BLE001 -- reported through the engine status
                err.append(e)
                return 1
        fn = GRAD_READY_FN(_ready)
        grad_hook.begin(dflat)
        ok = False
        try:
            check(L.spff_plan_set_grad_hook(self._h, fn, None), "spff_plan_set_grad_hook")
            try:
                rc = L.spff_backward(self._h, _ptr(dlogits_cl), _ptr(flat), _ptr(dflat), _ptr(ws),
                                     _stream(dlogits_cl.device))
            finally:
                L.spff_plan_set_grad_hook(self._h, GRAD_READY_FN(), None)
            if err:
                raise SpffError(f"gradient hook failed: {err[0]!r}") from err[0]
            self._check(rc, "spff_backward")
            if covered[0] != self.nfloats:
                raise SpffError(f"gradient hook covered {covered[0]} of {self.nfloats} floats")
            grad_hook.finish()
            ok = True
        finally:
            if not ok and hasattr(grad_hook, "abort"):
                # join the bucket all-reduces already issued, so peers that issued the
                # same ones complete them, then let the error propagate (the process
                # group's timeout ends any collective a peer is left waiting in)
                grad_hook.abort()
        return dflat

    def streams_head(self) -> bool:
        """The streaming head covers this plan (gemm.hip head_streams: base 32 or 64, K <= 32):
        predict then never writes the logits unless asked."""
        return (self.cfg.base in (32, 64) and 1 <= self.cfg.num_classes <= 32
                and os.environ.get("SPFF_HEAD_STREAM", "1")[:1] != "0")

    def predict(self, x: torch.Tensor, flat: torch.Tensor, labels: Optional[torch.Tensor] = None,
                ignore_index: Optional[int] = None, want_logits: bool = False):
        """spff_predict: x [B,Cin,D,H,W] -> (mask uint8 [B,D,H,W], conf int64 [K,K+1] or None,
        logits channel-last [B,D,H,W,K] or None).  ``labels`` [B,D,H,W]: also the confusion
        counts, as confusion() of the same logits (``ignore_index`` None: no voxel masked).
        Where the streaming head does not cover the plan the logits are allocated here (the
        row-argmax pass reads them) and returned only when ``want_logits``."""
        c = self.cfg
        require_device(x, f"{self.NAME} predict")
        if tuple(x.shape) != (c.batch, c.in_ch, c.depth, c.height, c.width):
            raise SpffError(f"input shape {tuple(x.shape)} does not match plan")
        if x.dtype != torch.float32:
            raise SpffError("the engine computes in fp32; got " + str(x.dtype))
        x = x.contiguous()
        dev, K = x.device, c.num_classes
        vol = (c.batch, c.depth, c.height, c.width)
        mask = torch.empty(vol, dtype=torch.uint8, device=dev)
        logits = conf = None
        if want_logits or not self.streams_head():
            logits = torch.empty(vol + (K,), dtype=torch.float32, device=dev)
        if labels is not None:
            labels = labels.to(device=dev, dtype=torch.int64).contiguous()
            if labels.numel() != mask.numel():
                raise SpffError(f"labels {tuple(labels.shape)} do not match the volume {vol}")
            conf = torch.empty(K * (K + 1), dtype=torch.int64, device=dev)
        ws = self.workspace(dev)
        self.generation += 1
        self.coll_error = None
        self._check(lib().spff_predict(self._h, _ptr(x), _ptr(flat), _ptr(mask), _ptr(logits),
                                       _ptr(labels), *_ignore_args(ignore_index), _ptr(conf),
                                       _ptr(ws), _stream(dev)), "spff_predict")
        return (mask, None if conf is None else conf.view(K, K + 1),
                logits if want_logits else None)

    PROF_CLASSES = ("conv_fwd", "conv_dgrad", "conv_wgrad", "gemm", "slab_reduce", "act_apply",
                    "in_bwd_apply", "f16_absmax")
    MEM_CLASSES = ("slab_reduce", "act_apply", "in_bwd_apply", "f16_absmax")

    def prof_enable(self, on: bool = True):
        check(lib().spff_prof_enable(self._h, int(bool(on))), "spff_prof_enable")

    def prof_collect(self) -> Dict[str, Tuple[float, float, int, float]]:
        """{class: (total_ms, algorithmic_flops, launches, compulsory_bytes)} since the last
        collect."""
        n = len(self.PROF_CLASSES)
        buf = (ctypes.c_double * (4 * n))()
        check(lib().spff_prof_collect(self._h, buf, n), "spff_prof_collect")
        return {c: (buf[4 * i], buf[4 * i + 1], int(buf[4 * i + 2]), buf[4 * i + 3])
                for i, c in enumerate(self.PROF_CLASSES)}

    def debug_set(self, key: int, value: int):
        """spff_debug_set (include/spff.h has the full account).
        key 0: stop the backward after N blocks -- 1, 2, 3 = dec1, dec2, dec3, 4 = bott,
        5 = enc3, 6 = enc2; -1 (default), 0 or 7 = the whole backward.
        key 1: store the GEMM-applied block outputs too (saved("dec1.out") etc.).
        key 2 = 0: the encoder output gradients by a k_maxpool_bwd_add pass instead of PoolAdd
        in their readers.
        key 3 = 0: conv1's IN-backward sums by a slab_reduce pass instead of the dgrad epilogue.
        key 4 = 0: the head's backward as passes of its own instead of folded into dec1's.
        key 5 = 1: the forward runs the head alone on the previous forward's workspace.
        After a stop, saved("grad.dy2") / saved("grad.da1") hold that block's gradients at y2 /
        y1, saved("grad.dx") its input gradient (decoder blocks: the up-conv half; the skip
        half is saved("grad.dskip<l>")), saved("grad.out") the gradient at the output of
        dec3, dec2 or bott (dec1: only with key 4 = 0); each grad.* view is [V0, base] and a
        level-l tensor its flat prefix [V_l, C_l]."""
        check(lib().spff_debug_set(self._h, int(key), int(value)), "spff_debug_set")

    def saved(self, name: str) -> torch.Tensor:
        """As _PlanBase.saved; uint8 for the max-pool argmax bytes "poolN.idx", int32 for the
        spatial attention's channel argmax "<stage>.sa.idx"."""
        if name.endswith(".sa.idx"):
            b, nv, ch = self._saved_view(name)
            return b[:4 * nv * ch].view(torch.int32).view(nv, ch).clone()
        if name.endswith(".idx"):
            b, nv, ch = self._saved_view(name)
            return b[:nv * ch].view(nv, ch).clone()
        return super().saved(name)


# Plans (and the workspace each pins: ~2.6 KB per voxel) belong to the module
# that created them: a small LRU of shapes per (module, tag) -- so alternating
# shapes (a partial last batch, validation at another size) do not rebuild and
# re-allocate a multi-GB workspace on every switch -- dropped with the module (weak
# keys), or explicitly by release_plans().  At most PLAN_CACHE plans per (module,
# tag), and older ones are evicted first while their workspaces together would exceed
# PLAN_CACHE_FRACTION of the device memory (a 5 x 512^3 plan alone is 211 GiB).
_OWNER_PLANS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_ANON_PLANS: Dict[tuple, object] = {}
PLAN_CACHE = int(os.environ.get("SPFF_PLAN_CACHE", "3"))
PLAN_CACHE_FRACTION = 0.4


def _all_plans():
    for slots in list(_OWNER_PLANS.values()):
        for lru in slots.values():
            yield from list(lru.values())
    yield from list(_ANON_PLANS.values())


def release_workspace(plan) -> None:
    """Free a cached plan's workspace (the plan stays; the next forward allocates a new
    one).  A backward still pending on that workspace's activations then fails loudly
    (its plan generation no longer matches) instead of reading freed memory."""
    if getattr(plan, "_ws", None) is not None:
        plan._ws = None
        plan.generation = getattr(plan, "generation", 0) + 1


def _alloc_workspace(plan, device) -> torch.Tensor:
    """The plan's workspace.  If the device is out of memory, the workspaces of the OTHER
    cached plans on the same device (validation shapes, a partial last batch: see
    _owned_plan) are released, torch's cache is emptied and the allocation retried:
    first only plans with no backward pending on their workspace (``_pending_gen``, set
    by the engine ops' autograd forward, cleared by their backward), then, as a last
    resort, those too (their pending backward then fails loudly, see release_workspace).
    A failure after that raises.  SPFF_PLAN_CACHE=1 keeps one plan per module and tag
    (round 2's behaviour: the previous shape's workspace is freed before a new shape's
    is built)."""
    device = torch.device(device)
    try:
        return torch.empty(plan.ws_bytes, dtype=torch.uint8, device=device)
    except torch.OutOfMemoryError:
        pass

    def same_device(q):
        ws = getattr(q, "_ws", None)
        return ws is not None and ws.device == device

    for last_resort in (False, True):
        for q in _all_plans():
            if q is plan or not same_device(q):
                continue
            if not last_resort and getattr(q, "_pending_gen", None) == getattr(q, "generation", 0):
                continue
            release_workspace(q)
        torch.cuda.empty_cache()
        try:
            return torch.empty(plan.ws_bytes, dtype=torch.uint8, device=device)
        except torch.OutOfMemoryError:
            if last_resort:
                raise


def _device_bytes() -> int:
    try:
        if torch.cuda.is_available():
            return int(torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory)
    except Exception:  # noqa: BLE001
        pass
    return 64 << 30


def _owned_plan(owner, tag: str, key: tuple, make):
    if owner is None:
        if key not in _ANON_PLANS:
            _ANON_PLANS[key] = make()
        return _ANON_PLANS[key]
    slots = _OWNER_PLANS.get(owner)
    if slots is None:
        slots = {}
        _OWNER_PLANS[owner] = slots
    lru = slots.setdefault(tag, collections.OrderedDict())
    if key in lru:
        lru.move_to_end(key)
        return lru[key]
    plan = make()  # host-side only: the workspace is allocated at first use
    budget = PLAN_CACHE_FRACTION * _device_bytes()
    while lru and (len(lru) >= PLAN_CACHE or
                   sum(getattr(q, "ws_bytes", 0) for q in lru.values())
                   + getattr(plan, "ws_bytes", 0) > budget):
        lru.popitem(last=False)  # free the least recently used plan's workspace first
    lru[key] = plan
    return plan


def release_plans(owner=None) -> None:
    """Drop the engine plans (and workspaces) of ``owner`` -- every module-owned
    and anonymous plan when owner is None."""
    if owner is None:
        _OWNER_PLANS.clear()
        _ANON_PLANS.clear()
    else:
        _OWNER_PLANS.pop(owner, None)


def shard_key(shard) -> Tuple[int, int, int]:
    """(world, rank[, axis]) -> (world, rank, axis); axis 0 = depth, 1 = height"""
    sh = tuple(int(v) for v in shard)
    return sh if len(sh) == 3 else (sh[0], sh[1], 0)


def get_plan(owner=None, tag: str = "", **kw) -> Plan:
    """The plan of ``owner`` (an nn.Module) for tag ``tag`` and this shape/flag set."""
    key = (kw["batch"], kw["in_ch"], kw["depth"], kw["height"], kw["width"], kw["num_classes"],
           kw.get("base", 32), kw.get("ksd", 3), bool(kw.get("efilm", True)),
           bool(kw.get("fgate", True)), bool(kw.get("se", True)), bool(kw.get("specse", True)),
           kw.get("math") or default_math(), shard_key(kw.get("shard", (1, 0))),
           kw.get("memory") or default_memory(), int(kw.get("efilm_hidden", 32)),
           int(kw.get("efilm_pe_dims", 16)), bool(kw.get("fgate_learn_phase", False)),
           bool(kw.get("spatial", False)), bool(kw.get("skip_gate", False)))

    def make():
        kk = dict(kw)
        kk["shard_world"], kk["shard_rank"], kk["shard_axis"] = shard_key(kk.pop("shard", (1, 0)))
        return Plan(**kk)
    return _owned_plan(owner, tag, key, make)


class UNet3DPlan(_PlanBase):
    """Engine plan of the 3DUNet baseline variant (include/spff.h spff_unet3d_*):
    Cicek3DUNet + the depth adapter of LitCicek3DUNet_DepthAdapter_Published
    (reference models.py:718-777).  Parameters are one flat fp32 buffer in
    reference state-dict order (``params``), BatchNorm running statistics a
    second one (``buffers``)."""

    PREFIX, CFG, NAME = "spff_unet3d", spff_unet3d_cfg, "3DUNet"

    def __init__(self, batch, in_ch, depth, height, width, num_classes, base=32, target_depth=0,
                 device=None, math=None):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math,
                         base=base, target_depth=target_depth)
        L, h = lib(), self._h
        self.buffers: List[Tuple[str, int, int]] = []
        for i in range(L.spff_unet3d_num_buffers(h)):
            name, off, n = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
            check(L.spff_unet3d_buffer_info(h, i, ctypes.byref(name), ctypes.byref(off),
                                            ctypes.byref(n)), "spff_unet3d_buffer_info")
            self.buffers.append((name.value.decode(), off.value, n.value))
        self.nbuf = int(L.spff_unet3d_buffer_floats(h))

    def _fill_cfg(self, cfg, base, target_depth):
        cfg.base, cfg.target_depth = base, int(target_depth)

    def set_sync_bn(self, impl) -> None:
        """Synchronised BatchNorm over a data-parallel group (spff_unet3d_set_sync_bn):
        ``impl`` has ``allreduce(t)`` (in-place sum of a device tensor over the group) and
        ``world``, e.g. innovative3D.sharded.TorchDepthColl; None restores per-replica
        statistics."""
        L = lib()
        if impl is None or int(getattr(impl, "world", 1)) <= 1:
            check(L.spff_unet3d_set_sync_bn(self._h, None, 1), "spff_unet3d_set_sync_bn")
            self._sync = None
            return

        def _allreduce(ctx, buf, n, dt, stream):
            try:
                ws = self._ws
                off = buf - ws.data_ptr()
                esz = 8 if dt == 1 else 4
                if off < 0 or off % esz or off + n * esz > ws.numel():
                    raise SpffError("collective buffer outside the plan workspace")
                t = ws[off:off + n * esz].view(torch.float64 if dt == 1 else torch.float32)
                cur = torch.cuda.current_stream(t.device)
                if stream and stream != cur.cuda_stream:
                    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=t.device)):
                        impl.allreduce(t)
                else:
                    impl.allreduce(t)
                return 0
            except Exception as e:  # noqa: BLE001 -- reported through the engine status
                self.coll_error = e
                return 1

        def _no_halo(ctx, interior, sl, d_local, stream):
            return 1
        self._sync_fns = (ALLREDUCE_FN(_allreduce), HALO_FN(_no_halo))  # keep alive
        self._sync = spff_coll(None, self._sync_fns[0], self._sync_fns[1])
        self.coll_error = None
        check(L.spff_unet3d_set_sync_bn(self._h, ctypes.byref(self._sync), int(impl.world)),
              "spff_unet3d_set_sync_bn")

    def forward(self, x: torch.Tensor, flat: torch.Tensor, bufs: torch.Tensor, training: bool,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B,Cin,D,H,W] fp32 -> logits channel-last [B,D,H,W,K]; training updates bufs."""
        return self._forward(x, flat, out, _ptr(bufs), int(bool(training)))


def _get_variant_plan(cls, owner, tag: str, kw: dict):
    """The plan of class ``cls`` for ``owner`` / ``tag`` (owned like get_plan); the cache key
    is the constructor's arguments with its declared defaults filled in."""
    args = inspect.signature(cls.__init__).bind(None, **kw)
    args.apply_defaults()
    args.arguments["math"] = kw.get("math") or default_math()
    kind = cls.PREFIX[len("spff_"):]
    key = (kind,) + tuple(tuple(v) if isinstance(v, (list, tuple)) else v
                          for n, v in args.arguments.items() if n not in ("self", "device"))
    return _owned_plan(owner, kind + ":" + tag, key, lambda: cls(**kw))


def get_unet3d_plan(owner=None, tag: str = "", **kw) -> UNet3DPlan:
    return _get_variant_plan(UNet3DPlan, owner, tag, kw)


class SwinPlan(_PlanBase):
    """One spff_swin plan (SwinUNETR variant) + its workspace."""

    PREFIX, CFG, NAME = "spff_swin", spff_swin_cfg, "SwinUNETR"

    def __init__(self, batch, in_ch, depth, height, width, num_classes, feature_size=12,
                 window=7, heads=(1, 2, 4, 8), mlp_ratio=2.0, device=None, math=None):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math,
                         feature_size=feature_size, window=window, heads=heads,
                         mlp_ratio=mlp_ratio)

    def _fill_cfg(self, cfg, feature_size, window, heads, mlp_ratio):
        cfg.feature_size, cfg.window, cfg.mlp_ratio = feature_size, window, float(mlp_ratio)
        for i, h in enumerate(heads):
            cfg.heads[i] = int(h)


def get_swin_plan(owner=None, tag: str = "", **kw) -> SwinPlan:
    return _get_variant_plan(SwinPlan, owner, tag, kw)


class UNETRPlan(_PlanBase):
    """One spff_unetr plan (UNETR variant) + its workspace.  The plan's input is the padded
    volume [B, Cin, depth, height, width]; when that differs from ``img`` the engine resamples
    to ``img`` and the logits back."""

    PREFIX, CFG, NAME = "spff_unetr", spff_unetr_cfg, "UNETR"

    def __init__(self, batch, in_ch, depth, height, width, num_classes, img=(96, 96, 96),
                 feature_size=16, hidden=768, mlp_dim=3072, heads=12, device=None, math=None):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math, img=img,
                         feature_size=feature_size, hidden=hidden, mlp_dim=mlp_dim, heads=heads)

    def _fill_cfg(self, cfg, img, feature_size, hidden, mlp_dim, heads):
        for i, v in enumerate(img):
            cfg.img[i] = int(v)
        cfg.feature_size, cfg.hidden, cfg.mlp_dim, cfg.heads = feature_size, hidden, mlp_dim, heads


def get_unetr_plan(owner=None, tag: str = "", **kw) -> UNETRPlan:
    return _get_variant_plan(UNETRPlan, owner, tag, kw)


def _vit_shape(qkv: torch.Tensor, batch: int, heads: int) -> Tuple[int, int]:
    """(tokens per sample, hidden) of qkv [batch * n, 3 * hidden]."""
    if qkv.ndim != 2 or qkv.dtype != torch.float32 or batch < 1 or heads < 1 \
            or qkv.shape[0] % batch or qkv.shape[1] % (3 * heads):
        raise SpffError(f"qkv must be fp32 [batch * n, 3 * heads * d]; got {qkv.dtype} "
                        f"{tuple(qkv.shape)} for batch {batch}, heads {heads}")
    return qkv.shape[0] // batch, qkv.shape[1] // 3


def vit_attn_fwd(qkv: torch.Tensor, batch: int, heads: int):
    """qkv [B*n, 3C] fp32, split as (qkv, head, d) -> (O [B*n, C], lse [B, heads, n])."""
    require_device(qkv, "vit_attn_fwd")
    qkv = qkv.contiguous()
    n, C = _vit_shape(qkv, batch, heads)
    T = batch * n
    O = torch.empty((T, C), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((batch, heads, n), dtype=torch.float32, device=qkv.device)
    check(lib().spff_vit_attn_fwd(_ptr(qkv), batch, n, C, heads, _ptr(O), _ptr(lse),
                                  _stream(qkv.device)), "spff_vit_attn_fwd")
    return O, lse


def vit_attn_bwd(qkv: torch.Tensor, O: torch.Tensor, dO: torch.Tensor, lse: torch.Tensor,
                 batch: int, heads: int) -> torch.Tensor:
    """-> dqkv [B*n, 3C] (every entry written)."""
    require_device(qkv, "vit_attn_bwd")
    qkv, O, dO, lse = qkv.contiguous(), O.contiguous(), dO.contiguous(), lse.contiguous()
    n, C = _vit_shape(qkv, batch, heads)
    for what, t, shape in (("O", O, (batch * n, C)), ("dO", dO, (batch * n, C)),
                           ("lse", lse, (batch, heads, n))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != qkv.device:
            raise SpffError(f"vit_attn_bwd: {what} must be fp32 {shape} on {qkv.device}; got "
                            f"{t.dtype} {tuple(t.shape)} on {t.device}")
    dqkv = torch.empty_like(qkv)
    ws = torch.empty(max(4, int(lib().spff_vit_attn_ws_bytes(batch, n, heads))), dtype=torch.uint8,
                     device=qkv.device)
    check(lib().spff_vit_attn_bwd(_ptr(qkv), _ptr(O), _ptr(dO), _ptr(lse), batch, n, C, heads,
                                  _ptr(dqkv), _ptr(ws), _stream(qkv.device)), "spff_vit_attn_bwd")
    return dqkv


def resize3d_fwd(x_cl: torch.Tensor, size) -> torch.Tensor:
    """x [B, D, H, W, C] channel-last fp32 -> [B, *size, C] (F.interpolate trilinear,
    align_corners=False)."""
    require_device(x_cl, "resize3d_fwd")
    if x_cl.ndim != 5 or x_cl.dtype != torch.float32:
        raise SpffError(f"resize3d_fwd: expected fp32 [B, D, H, W, C]; got {x_cl.dtype} "
                        f"{tuple(x_cl.shape)}")
    x_cl = x_cl.contiguous()
    B, D, H, W, C = x_cl.shape
    if len(tuple(size)) != 3 or min(int(v) for v in size) < 1:
        raise SpffError(f"resize3d_fwd: size must be three positive sizes; got {size}")
    Do, Ho, Wo = (int(v) for v in size)
    y = torch.empty((B, Do, Ho, Wo, C), dtype=torch.float32, device=x_cl.device)
    check(lib().spff_resize3d_fwd(_ptr(x_cl), _ptr(y), B, C, D, H, W, Do, Ho, Wo,
                                  _stream(x_cl.device)), "spff_resize3d_fwd")
    return y


def resize3d_bwd(dy_cl: torch.Tensor, in_size) -> torch.Tensor:
    """The adjoint of resize3d_fwd: dy [B, Do, Ho, Wo, C] -> dx [B, *in_size, C]."""
    require_device(dy_cl, "resize3d_bwd")
    if dy_cl.ndim != 5 or dy_cl.dtype != torch.float32:
        raise SpffError(f"resize3d_bwd: expected fp32 [B, D, H, W, C]; got {dy_cl.dtype} "
                        f"{tuple(dy_cl.shape)}")
    dy_cl = dy_cl.contiguous()
    B, Do, Ho, Wo, C = dy_cl.shape
    if len(tuple(in_size)) != 3 or min(int(v) for v in in_size) < 1:
        raise SpffError(f"resize3d_bwd: in_size must be three positive sizes; got {in_size}")
    D, H, W = (int(v) for v in in_size)
    dx = torch.empty((B, D, H, W, C), dtype=torch.float32, device=dy_cl.device)
    check(lib().spff_resize3d_bwd(_ptr(dy_cl), _ptr(dx), B, C, D, H, W, Do, Ho, Wo,
                                  _stream(dy_cl.device)), "spff_resize3d_bwd")
    return dx


def _sa_rows(what: str, x_cl: torch.Tensor) -> Tuple[int, int, int, int, int]:
    require_device(x_cl, what)
    if x_cl.ndim != 5 or x_cl.dtype != torch.float32 or x_cl.shape[4] % 8 or not x_cl.numel():
        raise SpffError(f"{what}: expected fp32 [B, D, H, W, C] with C a multiple of 8; got "
                        f"{x_cl.dtype} {tuple(x_cl.shape)}")
    return tuple(int(v) for v in x_cl.shape)


def _sa_weight(what: str, w: torch.Tensor, device) -> torch.Tensor:
    if tuple(w.shape) != (1, 2, 3, 7, 7) or w.dtype != torch.float32 or w.device != device:
        raise SpffError(f"{what}: conv.weight must be fp32 [1, 2, 3, 7, 7] on {device}; got "
                        f"{w.dtype} {tuple(w.shape)} on {w.device}")
    return w.contiguous()


def spatial_attn_fwd(x_cl: torch.Tensor, w: torch.Tensor):
    """CBAM spatial attention (reference SpatialAttention3D) of channel-last fp32
    x [B, D, H, W, C] with conv.weight w [1, 2, 3, 7, 7] -> (y = x * attn, attn [B, D, H, W],
    map [B, D, H, W, 2] = (channel mean, channel max), idx [B, D, H, W] int32 = the lowest
    channel that holds the max)."""
    B, D, H, W, C = _sa_rows("spatial_attn_fwd", x_cl)
    x_cl, dev = x_cl.contiguous(), x_cl.device
    w = _sa_weight("spatial_attn_fwd", w, dev)
    y = torch.empty_like(x_cl)
    attn = torch.empty((B, D, H, W), dtype=torch.float32, device=dev)
    amap = torch.empty((B, D, H, W, 2), dtype=torch.float32, device=dev)
    idx = torch.empty((B, D, H, W), dtype=torch.int32, device=dev)
    check(lib().spff_spatial_attn_fwd(_ptr(x_cl), _ptr(w), B, D, H, W, C, _ptr(y), _ptr(attn),
                                      _ptr(amap), _ptr(idx), None, _stream(dev)),
          "spff_spatial_attn_fwd")
    return y, attn, amap, idx


def spatial_attn_bwd(dy_cl: torch.Tensor, x_cl: torch.Tensor, w: torch.Tensor,
                     attn: torch.Tensor, amap: torch.Tensor, idx: torch.Tensor):
    """The backward of spatial_attn_fwd from what it returned: -> (dx like x, dw like w)."""
    B, D, H, W, C = _sa_rows("spatial_attn_bwd", x_cl)
    x_cl, dev = x_cl.contiguous(), x_cl.device
    w = _sa_weight("spatial_attn_bwd", w, dev)
    for what, t, shape, dt in (("dy", dy_cl, (B, D, H, W, C), torch.float32),
                               ("attn", attn, (B, D, H, W), torch.float32),
                               ("map", amap, (B, D, H, W, 2), torch.float32),
                               ("idx", idx, (B, D, H, W), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
            raise SpffError(f"spatial_attn_bwd: {what} must be {dt} {shape} on {dev}; got "
                            f"{t.dtype} {tuple(t.shape)} on {t.device}")
    dy_cl, attn, amap, idx = dy_cl.contiguous(), attn.contiguous(), amap.contiguous(), \
        idx.contiguous()
    dx = torch.empty_like(x_cl)
    dw = torch.empty_like(w)
    ws = torch.empty(int(lib().spff_spatial_attn_ws_bytes(B, D, H, W, C)), dtype=torch.uint8,
                     device=dev)
    check(lib().spff_spatial_attn_bwd(_ptr(dy_cl), _ptr(x_cl), _ptr(w), _ptr(attn), _ptr(amap),
                                      _ptr(idx), B, D, H, W, C, _ptr(dx), _ptr(dw), _ptr(ws),
                                      _stream(dev)), "spff_spatial_attn_bwd")
    return dx, dw


class R2UPlan(_PlanBase):
    """Engine plan of the R2UNet3D variant (include/spff.h spff_r2u_*): the recurrent
    residual U-Net backbone + 1x1x1 head of LitR2UNet3D_Published.  Parameters are one
    flat fp32 buffer in the Lit module's state-dict order and names (``params``); D, H
    and W are multiples of 16 (the wrapper pads and crops)."""

    PREFIX, CFG, NAME = "spff_r2u", spff_r2u_cfg, "R2UNet3D"

    def __init__(self, batch, in_ch, depth, height, width, num_classes, base=16, t=2,
                 device=None, math=None):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math,
                         base=base, t=t)

    def _fill_cfg(self, cfg, base, t):
        cfg.base, cfg.t = base, int(t)


def get_r2u_plan(owner=None, tag: str = "", **kw) -> R2UPlan:
    return _get_variant_plan(R2UPlan, owner, tag, kw)


class RUPPPlan(_PlanBase):
    """Engine plan of the ResUNet++ variant (include/spff.h spff_rupp_*): residual units,
    ASPP bottleneck, SE and attention-gated skips + the 1x1x1 head of
    LitResUNetPP3D_Published.  Parameters are one flat fp32 buffer in the Lit module's
    named_parameters() order and names (``params``); D, H and W are multiples of 16 (the
    wrapper pads and crops)."""

    PREFIX, CFG, NAME = "spff_rupp", spff_rupp_cfg, "ResUNet++"

    def __init__(self, batch, in_ch, depth, height, width, num_classes, base=16,
                 device=None, math=None):
        super().__init__(batch, in_ch, depth, height, width, num_classes, device, math, base=base)

    def _fill_cfg(self, cfg, base):
        cfg.base = base


def get_rupp_plan(owner=None, tag: str = "", **kw) -> RUPPPlan:
    return _get_variant_plan(RUPPPlan, owner, tag, kw)


# ------------------------------------------------------------- data path ops --
def rasterize_ellipses(rois: torch.Tensor, frames: int, height: int, width: int) -> torch.Tensor:
    """rois [n, 5] int32 (x0, y0, w0, h0, label) on the device -> labels [F, H, W] int64."""
    require_device(rois, "rasterize_ellipses")
    rois = rois.to(torch.int32).contiguous()
    lab = torch.empty((frames, height, width), dtype=torch.int64, device=rois.device)
    check(lib().spff_rasterize_ellipses(_ptr(rois), rois.shape[0], frames, height, width,
                                        _ptr(lab), _stream(rois.device)), "spff_rasterize_ellipses")
    return lab


def resize_bilinear_aa(frames: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """[N, h, w] fp32 -> [N, height, width] (F.interpolate bilinear, antialias)."""
    require_device(frames, "resize_bilinear_aa")
    x = frames.to(torch.float32).contiguous()
    n, hin, win = x.shape
    out = torch.empty((n, height, width), dtype=torch.float32, device=x.device)
    tmp = torch.empty((n, hin, width), dtype=torch.float32, device=x.device)
    check(lib().spff_resize_bilinear_aa(_ptr(x), n, hin, win, _ptr(out), height, width, _ptr(tmp),
                                        _stream(x.device)), "spff_resize_bilinear_aa")
    return out


def grid_aug(x: torch.Tensor, y: Optional[torch.Tensor], maps: torch.Tensor, prm: torch.Tensor,
             seed: int, out_hw) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """x [B,F,H,W] fp32 (+ y int64) -> augmented [B,F,Ho,Wo]; maps [B,H+W] int32 and
    prm [B,8] fp32 on the device (see include/spff.h spff_grid_aug)."""
    require_device(x, "grid_aug")
    x = x.contiguous()
    B, F_, H, W = x.shape
    Ho, Wo = out_hw
    xo = torch.empty((B, F_, Ho, Wo), dtype=torch.float32, device=x.device)
    yo = None
    if y is not None:
        y = y.to(device=x.device, dtype=torch.int64).contiguous()
        yo = torch.empty((B, F_, Ho, Wo), dtype=torch.int64, device=x.device)
    ws = torch.empty(int(lib().spff_grid_aug_ws_bytes(B)), dtype=torch.uint8, device=x.device)
    check(lib().spff_grid_aug(_ptr(x), _ptr(y), B, F_, H, W, _ptr(maps.contiguous()),
                              _ptr(prm.contiguous()), ctypes.c_uint64(int(seed) & (2**64 - 1)),
                              _ptr(xo), _ptr(yo), _ptr(ws), _stream(x.device)), "spff_grid_aug")
    return xo, yo


# ------------------------------------------------------------------ loss ops --
def loss_ws(device) -> torch.Tensor:
    n = int(lib().spff_loss_ws_bytes(0, 1))
    return torch.empty(n, dtype=torch.uint8, device=device)


def _loss_io(what: str, logits_cl: torch.Tensor, labels: torch.Tensor, K: int):
    """A loss op's inputs as the kernels read them and its outputs: (contiguous logits rows,
    int64 labels on their device, out4, dlogits_cl)."""
    require_device(logits_cl, what)
    logits_cl = logits_cl.contiguous()
    labels = labels.to(device=logits_cl.device, dtype=torch.int64).contiguous()
    if logits_cl.numel() != labels.numel() * K:
        raise SpffError(f"logits ({tuple(logits_cl.shape)}) / labels ({tuple(labels.shape)}) mismatch")
    out4 = torch.empty(4, dtype=torch.float32, device=logits_cl.device)
    return logits_cl, labels, out4, torch.empty_like(logits_cl)


def _ce_loss(what: str, entry: str, logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
             ignore_index: int, smooth: float, count_override: Optional[torch.Tensor], *mid):
    """spff_loss / spff_loss_ex (``mid``: the latter's arguments between count_override and
    out4): returns (out4, dlogits_cl, conf[K, K+1])."""
    logits_cl, labels, out4, dl = _loss_io(what, logits_cl, labels, K)
    dev = logits_cl.device
    conf = torch.empty(K * (K + 1), dtype=torch.int64, device=dev)
    ws = loss_ws(dev)
    check(getattr(lib(), entry)(_ptr(logits_cl), _ptr(labels), labels.numel(), K,
                                int(ignore_index), float(smooth), _ptr(count_override), *mid,
                                _ptr(out4), _ptr(dl), _ptr(conf), _ptr(ws), _stream(dev)), entry)
    return out4, dl, conf.view(K, K + 1)


def ce_dice_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int, ignore_index: int,
                    smooth: float, count_override: Optional[torch.Tensor] = None):
    """Returns (out4, dlogits_cl, conf[K, K+1])."""
    return _ce_loss("ce_plus_macro_dice_loss", "spff_loss", logits_cl, labels, K, ignore_index,
                    smooth, count_override)


def weighted_ce_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int, ignore_index: int,
                        class_weights: Optional[torch.Tensor] = None,
                        count_override: Optional[torch.Tensor] = None):
    """The 3DUNet wrapper's _weighted_softmax_ce (models.py:779-799):
    sum_v w[y_v] nll_v / max(N_valid, 1).  Returns (out4, dlogits_cl, conf)."""
    cw = None
    if class_weights is not None:
        cw = class_weights.to(device=logits_cl.device, dtype=torch.float32).contiguous()
        if cw.numel() != K:
            raise SpffError(f"class_weights has {cw.numel()} entries, expected {K}")
    return _ce_loss("weighted softmax CE", "spff_loss_ex", logits_cl, labels, K, ignore_index,
                    1e-6, count_override, _ptr(cw), 1)


def _variant_loss(what: str, entry: str, logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
                  *tail):
    """A variant's loss on the soft-Dice kernels (``entry`` and ``entry``_ws_bytes): returns
    (out4, dlogits_cl).  ``tail``: the loss's own arguments between K and out4."""
    logits_cl, labels, out4, dl = _loss_io(what + " loss", logits_cl, labels, K)
    B, V, dev = logits_cl.shape[0], labels.numel(), logits_cl.device
    if V % B:
        raise SpffError(f"logits ({tuple(logits_cl.shape)}) / labels ({tuple(labels.shape)}) mismatch")
    L = lib()
    ws = torch.empty(int(getattr(L, entry + "_ws_bytes")(B, K)), dtype=torch.uint8, device=dev)
    check(getattr(L, entry)(_ptr(logits_cl), _ptr(labels), B, V // B, K, *tail, _ptr(out4),
                            _ptr(dl), _ptr(ws), _stream(dev)), entry)
    return out4, dl


def _ignore_args(ignore_index: Optional[int]) -> Tuple[int, int]:
    """(use_ignore, ignore_index); None: no voxel is masked"""
    return int(ignore_index is not None), int(ignore_index) if ignore_index is not None else 0


def swin_loss_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int, ignore_index: int,
                      include_bg: bool, ce_weight: float):
    """LitSwinUNETR_Published._loss on the HIP kernels: returns (out4, dlogits_cl)."""
    return _variant_loss("SwinUNETR", "spff_swin_loss", logits_cl, labels, K, int(ignore_index),
                         int(bool(include_bg)), float(ce_weight))


def r2u_dice_loss_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
                          ignore_index: Optional[int]):
    """LitR2UNet3D_Published._dice_only_loss_with_logits (multi-class branch) on the HIP
    kernels: returns (out4 = [dice, loss, kept_samples, N_valid], dlogits_cl).
    ``ignore_index`` None: no voxel is masked."""
    return _variant_loss("R2UNet3D", "spff_r2u_dice_loss", logits_cl, labels, K,
                         *_ignore_args(ignore_index))


def rupp_loss_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
                      ignore_index: Optional[int], include_bg: bool = False,
                      ce_weight: float = 1.0, dice_weight: float = 1.0):
    """dice_ce_loss_with_metrics (LitResUNetPP3D_Published._loss) on the HIP kernels:
    returns (out4 = [ce, loss, dice_mean, N_valid], dlogits_cl).  Dice sums are pooled over
    the whole batch; ``ignore_index`` None: no voxel is masked."""
    return _variant_loss("ResUNet++", "spff_rupp_loss", logits_cl, labels, K,
                         *_ignore_args(ignore_index), int(bool(include_bg)), float(ce_weight),
                         float(dice_weight))


def unet3d_loss_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
                        ignore_index: Optional[int],
                        class_weights: Optional[torch.Tensor] = None,
                        voxel_weights: Optional[torch.Tensor] = None, include_bg: bool = False,
                        ce_weight: float = 1.0, dice_weight: float = 0.0):
    """The 3DUNet wrapper's _weighted_softmax_ce (per-class and per-voxel weights, denominator
    max(sum m u, 1)) + dice_weight times its per-sample _dice_loss, on the HIP kernels: returns
    (out4 = [ce, loss, dice_loss, sum m u], dlogits_cl).  ``voxel_weights``: one weight per
    label, in the labels' order; ``ignore_index`` None: no voxel is masked."""
    dev = logits_cl.device
    cw = vw = None
    if class_weights is not None:
        cw = class_weights.to(device=dev, dtype=torch.float32).contiguous()
        if cw.numel() != K:
            raise SpffError(f"class_weights has {cw.numel()} entries, expected {K}")
    if voxel_weights is not None:
        vw = voxel_weights.to(device=dev, dtype=torch.float32).contiguous()
        if vw.numel() != labels.numel():
            raise SpffError(f"voxel_weights ({tuple(vw.shape)}) / labels "
                            f"({tuple(labels.shape)}) mismatch")
    return _variant_loss("3DUNet", "spff_unet3d_loss", logits_cl, labels, K,
                         *_ignore_args(ignore_index), _ptr(cw), _ptr(vw), int(bool(include_bg)),
                         float(ce_weight), float(dice_weight))


def nnunet_loss_forward(logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
                        ignore_index: Optional[int] = -1, include_bg: bool = False,
                        ce_weight: float = 1.0, dice_weight: float = 1.0):
    """models.dice_ce_loss (nnU-Net style soft Dice with a squared-probability denominator,
    pooled over the batch, + mean CE) on the HIP kernels: returns
    (out4 = [ce, loss, dice_mean, N_valid], dlogits_cl)."""
    return _variant_loss("nnU-Net Dice+CE", "spff_nnunet_loss", logits_cl, labels, K,
                         *_ignore_args(ignore_index), int(bool(include_bg)), float(ce_weight),
                         float(dice_weight))


def confusion(logits_cl: torch.Tensor, labels: torch.Tensor, K: int,
              ignore_index: Optional[int]) -> torch.Tensor:
    require_device(logits_cl, "per_class_metrics_3d")
    logits_cl = logits_cl.contiguous()
    labels = labels.to(device=logits_cl.device, dtype=torch.int64).contiguous()
    conf = torch.empty(K * (K + 1), dtype=torch.int64, device=logits_cl.device)
    ign = -(2 ** 31) if ignore_index is None else int(ignore_index)
    check(lib().spff_confusion(_ptr(logits_cl), _ptr(labels), labels.numel(), K, ign, _ptr(conf),
                               _stream(logits_cl.device)), "spff_confusion")
    return conf.view(K, K + 1)


def rank_auc(scores_cl: torch.Tensor, labels: torch.Tensor, K: int, from_logits: bool,
             per_sample: bool) -> torch.Tensor:
    """spff_rank_auc on channel-last rows [B, ..., K]: a float64 device tensor [rows, 4] of
    (pr_auc, roc_auc, n_pos, n_neg) -- K + 1 rows (the micro row last), or B * K rows in
    (b, c) order when ``per_sample``.  No host sync."""
    require_device(scores_cl, "rank_auc")
    scores_cl = scores_cl.to(torch.float32).contiguous()
    B = scores_cl.shape[0]
    labels = labels.to(device=scores_cl.device, dtype=torch.int64).contiguous()
    V = labels.numel()
    if K < 1 or scores_cl.numel() != V * K or B < 1 or V % B:
        raise SpffError(f"scores ({tuple(scores_cl.shape)}) / labels ({tuple(labels.shape)}) "
                        f"mismatch for K = {K}")
    dev = scores_cl.device
    rows = B * K if per_sample else K + 1
    out = torch.empty((rows, 4), dtype=torch.float64, device=dev)
    L = lib()
    ws = torch.empty(max(1, int(L.spff_rank_auc_ws_bytes(B, V // B, K, int(bool(per_sample))))),
                     dtype=torch.uint8, device=dev)
    check(L.spff_rank_auc(_ptr(scores_cl), _ptr(labels), B, V // B, K, int(bool(from_logits)),
                          int(bool(per_sample)), _ptr(out), _ptr(ws), _stream(dev)),
          "spff_rank_auc")
    return out


def pred_views_ws_bytes(B: int, D: int, H: int, W: int, K: int) -> int:
    return int(lib().spff_pred_views_ws_bytes(B, D, H, W, K))


def pred_views(logits_cl: torch.Tensor, depth_split: int = 0, ws: Optional[torch.Tensor] = None):
    """spff_pred_views on channel-last logits [B, D, H, W, K]: (center_pred uint8 [B, H, W],
    alpha_center float [B, H, W], mip_prob float [B, H, W, K], mip_pred uint8 [B, H, W]) on
    the logits' device.  ``depth_split`` 0 leaves the split of the depth to the kernel;
    ``ws`` is a uint8 device tensor of at least pred_views_ws_bytes (allocated when None).
    No host sync."""
    require_device(logits_cl, "pred_views")
    if logits_cl.ndim != 5:
        raise SpffError(f"pred_views: expected [B, D, H, W, K] logits, got {tuple(logits_cl.shape)}")
    logits_cl = logits_cl.to(torch.float32).contiguous()
    B, D, H, W, K = (int(v) for v in logits_cl.shape)
    dev = logits_cl.device
    L = lib()
    need = int(L.spff_pred_views_ws_bytes(B, D, H, W, K))
    if ws is None:
        ws = torch.empty(max(1, need), dtype=torch.uint8, device=dev)
    elif ws.device != dev or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise SpffError(f"pred_views: ws must be a contiguous uint8 tensor of >= {need} bytes on {dev}")
    center_pred = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    alpha_center = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    mip_prob = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
    mip_pred = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    check(L.spff_pred_views(_ptr(logits_cl), B, D, H, W, K, int(depth_split), _ptr(center_pred),
                            _ptr(alpha_center), _ptr(mip_prob), _ptr(mip_pred), _ptr(ws),
                            _stream(dev)), "spff_pred_views")
    return center_pred, alpha_center, mip_prob, mip_pred


def input_views(x: torch.Tensor):
    """spff_input_views on x [B, C, D, H, W]: (center [B, H, W] = x[:, 0, D // 2],
    mip [B, H, W] = x[:, 0].amax(1), range [B, 4] = their (min, max) pairs).  No host sync."""
    require_device(x, "input_views")
    if x.ndim != 5:
        raise SpffError(f"input_views: expected [B, C, D, H, W], got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    B, C, D, H, W = (int(v) for v in x.shape)
    center = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    mip = torch.empty_like(center)
    rng = torch.empty((B, 4), dtype=torch.float32, device=x.device)
    check(lib().spff_input_views(_ptr(x), B, C, D, H, W, _ptr(center), _ptr(mip), _ptr(rng),
                                 _stream(x.device)), "spff_input_views")
    return center, mip, rng


def overlay_rgb(center: torch.Tensor, mip: torch.Tensor, rng: torch.Tensor,
                labels_center: Optional[torch.Tensor], center_pred: torch.Tensor,
                mip_pred: torch.Tensor, alpha_center: torch.Tensor, colors: torch.Tensor,
                K: int) -> torch.Tensor:
    """spff_overlay_rgb: the five-panel strip uint8 [B, H, 5 W, 3] from what input_views and
    pred_views return, the labels' centre slice [B, H, W] (or None) and a uint8 [256, 3]
    colour table.  No host sync."""
    require_device(center, "overlay_rgb")
    dev = center.device
    B, H, W = (int(v) for v in center.shape)

    def dev_t(t, dtype, shape, what):
        if tuple(t.shape) != shape:
            raise SpffError(f"overlay_rgb: {what} is {tuple(t.shape)}, expected {shape}")
        return t.to(device=dev, dtype=dtype).contiguous()

    center = dev_t(center, torch.float32, (B, H, W), "center")
    mip = dev_t(mip, torch.float32, (B, H, W), "mip")
    rng = dev_t(rng, torch.float32, (B, 4), "range")
    if labels_center is not None:
        labels_center = dev_t(labels_center, torch.int64, (B, H, W), "labels_center")
    center_pred = dev_t(center_pred, torch.uint8, (B, H, W), "center_pred")
    mip_pred = dev_t(mip_pred, torch.uint8, (B, H, W), "mip_pred")
    alpha_center = dev_t(alpha_center, torch.float32, (B, H, W), "alpha_center")
    colors = dev_t(colors, torch.uint8, (256, 3), "colors")
    rgb = torch.empty((B, H, 5 * W, 3), dtype=torch.uint8, device=dev)
    check(lib().spff_overlay_rgb(_ptr(center), _ptr(mip), _ptr(rng), _ptr(labels_center),
                                 _ptr(center_pred), _ptr(mip_pred), _ptr(alpha_center),
                                 _ptr(colors), B, H, W, int(K), _ptr(rgb), _stream(dev)),
          "spff_overlay_rgb")
    return rgb


def _tile_table(what: str, windows, n: Optional[int]):
    """The HOST window table [n][4] (z0, y0, x0, flip bits) as a C int32 array: its first
    ``n`` rows (None: all).  -> (array, n)"""
    rows = [[int(v) for v in row] for row in windows]
    n = len(rows) if n is None else int(n)
    if not 1 <= n <= len(rows) or any(len(r) != 4 for r in rows):
        raise SpffError(f"{what}: expected a window table [n][4] and 1 <= n <= {len(rows)}")
    return (ctypes.c_int32 * (4 * n))(*[v for r in rows[:n] for v in r]), n


def _tile_dev(what: str, t: torch.Tensor, name: str, dev, shape, dtype=torch.float32):
    if t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise SpffError(f"{what}: {name} must be a contiguous {dtype} tensor {tuple(shape)} on "
                        f"{dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def tile_gather(x: torch.Tensor, windows, roi, out: Optional[torch.Tensor] = None,
                n: Optional[int] = None) -> torch.Tensor:
    """spff_tile_gather: the first ``n`` windows of the table (None: all) of one volume x
    [C, D, H, W] into out[:n] of out [m >= n, C, rd, rh, rw] (allocated [n, ...] when None);
    a window with flip bits is gathered mirrored.  No host sync."""
    require_device(x, "tile_gather")
    if x.ndim != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise SpffError(f"tile_gather: expected a contiguous fp32 volume [C, D, H, W], got "
                        f"{x.dtype} {tuple(x.shape)}")
    tab, n = _tile_table("tile_gather", windows, n)
    C, D, H, W = (int(v) for v in x.shape)
    rd, rh, rw = (int(v) for v in roi)
    if out is None:
        out = torch.empty((n, C, rd, rh, rw), dtype=torch.float32, device=x.device)
    elif out.ndim != 5 or out.shape[0] < n:
        raise SpffError(f"tile_gather: out {tuple(out.shape)} holds fewer than {n} windows")
    _tile_dev("tile_gather", out, "out", x.device, (out.shape[0], C, rd, rh, rw))
    check(lib().spff_tile_gather(_ptr(x), C, D, H, W, tab, n, rd, rh, rw, _ptr(out),
                                 _stream(x.device)), "spff_tile_gather")
    return out


def tile_accumulate(tiles_cl: torch.Tensor, windows, weights, acc: torch.Tensor,
                    softmax: bool = False, n: Optional[int] = None) -> torch.Tensor:
    """spff_tile_accumulate: acc [D, H, W, K] += w s over the first ``n`` windows of the table
    (None: all), in table order; tiles_cl [m >= n, rd, rh, rw, K] channel-last window outputs,
    ``weights`` = (wz [rd], wy [rh], wx [rw]) fp32 device tensors; ``softmax``: s is the fp32
    softmax of the tile's row instead of its value.  In place; no host sync."""
    require_device(acc, "tile_accumulate")
    tab, n = _tile_table("tile_accumulate", windows, n)
    if acc.ndim != 4 or tiles_cl.ndim != 5 or tiles_cl.shape[0] < n:
        raise SpffError(f"tile_accumulate: acc {tuple(acc.shape)} / tiles {tuple(tiles_cl.shape)} "
                        f"for {n} windows")
    dev = acc.device
    D, H, W, K = (int(v) for v in acc.shape)
    m, rd, rh, rw = (int(v) for v in tiles_cl.shape[:4])
    _tile_dev("tile_accumulate", acc, "acc", dev, (D, H, W, K))
    _tile_dev("tile_accumulate", tiles_cl, "tiles", dev, (m, rd, rh, rw, K))
    wz, wy, wx = (_tile_dev("tile_accumulate", w, nm, dev, (r,))
                  for w, nm, r in zip(weights, ("wz", "wy", "wx"), (rd, rh, rw)))
    check(lib().spff_tile_accumulate(_ptr(tiles_cl), tab, n, rd, rh, rw, K, D, H, W, _ptr(wz),
                                     _ptr(wy), _ptr(wx), int(bool(softmax)), _ptr(acc),
                                     _stream(dev)), "spff_tile_accumulate")
    return acc


def tile_finalize(acc: torch.Tensor, norms=None, flips: int = 1,
                  labels: Optional[torch.Tensor] = None, ignore_index: Optional[int] = None,
                  scores=False, mask: Optional[torch.Tensor] = None,
                  conf: Optional[torch.Tensor] = None):
    """spff_tile_finalize on acc [D, H, W, K]: (mask uint8 [D, H, W] = the first maximum of
    every row, conf int64 [K, K + 1] as confusion() of the same rows or None without
    ``labels`` [D, H, W], scores or None).  ``scores``: False, True (a new tensor), or the
    tensor to write -- acc itself is allowed; scores = acc / (flips nz[z] ny[y] nx[x]) with
    ``norms`` = (nz [D], ny [H], nx [W]) fp32 device tensors.  ``mask`` / ``conf``: the
    tensors to write (allocated when None).  No host sync."""
    require_device(acc, "tile_finalize")
    if acc.ndim != 4:
        raise SpffError(f"tile_finalize: expected acc [D, H, W, K], got {tuple(acc.shape)}")
    dev = acc.device
    D, H, W, K = (int(v) for v in acc.shape)
    _tile_dev("tile_finalize", acc, "acc", dev, (D, H, W, K))
    if mask is None:
        mask = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    _tile_dev("tile_finalize", mask, "mask", dev, (D, H, W), torch.uint8)
    out_scores, nz, ny, nx = None, None, None, None
    if scores is not False and scores is not None:
        if norms is None:
            raise SpffError("tile_finalize: scores need the norm vectors")
        nz, ny, nx = (_tile_dev("tile_finalize", v, nm, dev, (r,))
                      for v, nm, r in zip(norms, ("nz", "ny", "nx"), (D, H, W)))
        out_scores = torch.empty_like(acc) if scores is True else scores
        _tile_dev("tile_finalize", out_scores, "scores", dev, (D, H, W, K))
    if labels is not None:
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
        if labels.numel() != D * H * W:
            raise SpffError(f"tile_finalize: labels {tuple(labels.shape)} do not match the "
                            f"volume {(D, H, W)}")
        if conf is None:
            conf = torch.empty(K * (K + 1), dtype=torch.int64, device=dev)
        _tile_dev("tile_finalize", conf, "conf", dev, (K * (K + 1),), torch.int64)
    else:
        conf = None
    check(lib().spff_tile_finalize(_ptr(acc), D, H, W, K, _ptr(nz), _ptr(ny), _ptr(nx),
                                   float(flips), _ptr(mask), _ptr(out_scores), _ptr(labels),
                                   *_ignore_args(ignore_index), _ptr(conf), _stream(dev)),
          "spff_tile_finalize")
    return mask, None if conf is None else conf.view(K, K + 1), out_scores


def count_valid(labels: torch.Tensor, ignore_index: int) -> torch.Tensor:
    require_device(labels, "count_valid")
    labels = labels.to(torch.int64).contiguous()
    cnt = torch.empty(1, dtype=torch.int64, device=labels.device)
    check(lib().spff_count_valid(_ptr(labels), labels.numel(), int(ignore_index), _ptr(cnt),
                                 _stream(labels.device)), "spff_count_valid")
    return cnt


def scale_(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    check(lib().spff_scale(_ptr(x), x.numel(), _ptr(scale.to(torch.float32).contiguous()),
                           _stream(x.device)), "spff_scale")
    return x


def to_channels_last(t: torch.Tensor) -> torch.Tensor:
    """[B,C,D,H,W] -> contiguous [B,D,H,W,C] (a free view for channels_last_3d)."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


CONV_PROF_CLASSES = ("conv_fwd", "conv_dgrad", "conv_wgrad", "loss_pass", "k_loss",
                     "unetr_vit", "unetr_resample")


def conv_prof_enable(on: bool = True) -> None:
    """Library-wide conv timing (every 3x3x3 conv launch of any plan; HIP events on the
    launch's stream) -- the 3DUNet / SwinUNETR bench lines' roofline source."""
    check(lib().spff_conv_prof_enable(int(bool(on))), "spff_conv_prof_enable")


def conv_prof_collect() -> Dict[str, Tuple[float, float, int]]:
    """{class: (ms, algorithmic fp32 flops, launches)} since the last enable / collect."""
    n = len(CONV_PROF_CLASSES)
    buf = (ctypes.c_double * (4 * n))()
    check(lib().spff_conv_prof_collect(buf, n), "spff_conv_prof_collect")
    return {c: (buf[4 * i], buf[4 * i + 1], int(buf[4 * i + 2]))
            for i, c in enumerate(CONV_PROF_CLASSES)}
