"""ctypes binding of libtextboost_hip.so (see include/textboost_hip.h). Fails loudly if the library is missing:
there is no CPU / eager fallback in the product path."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch  # noqa: F401  (must be imported first so libamdhip64.so.7 resolves to the runtime torch uses)

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libtextboost_hip" + os.environ.get("TB_LIB_SUFFIX", "") + ".so")
# the same sources compiled with -DTB_BF16: every 16-bit operand / activation is bfloat16 (the reference's --mixed_precision bf16)
LIB_PATH_BF16 = os.path.join(_PKG, "libtextboost_hip_bf16" + os.environ.get("TB_LIB_SUFFIX", "") + ".so")

TB_F16, TB_F32 = 0, 1
ACT_NONE, ACT_QUICK_GELU, ACT_GEGLU, ACT_SILU, ACT_QUICK_GELU_GRAD, ACT_GELU, ACT_GELU_GRAD, ACT_GEGLU_GRAD = 0, 1, 2, 3, 4, 5, 6, 7
ACT_LN_FWD, ACT_LN_BWD = 8, 9
(ST_LOSS_SCALE, ST_GROWTH_TRACKER, ST_STEP, ST_FOUND_INF, ST_COEF_LORA, ST_COEF_EMB, ST_BC1, ST_BC2, ST_GRAD_NORM,
 ST_SUMSQ_LORA, ST_SUMSQ_EMB, ST_LOSS_MSE, ST_LOSS_KPL, ST_LR_MULT, ST_LOSS_ATTN) = range(15)
ST_COUNT = 16
A_LINEAR, A_CONV3X3 = 0, 1
FREEU_SCALAR, FREEU_STRUCTURE = 0, 1

# {entry point: ([argtypes], restype)} and the descriptor structs (ctypes.Structure classes), read from include/textboost_hip.h
_STRUCTS, _SIGS = _abi.load()[:2]
GemmDesc, AttnDesc, FfDesc, ChainDesc, OptDesc = (_STRUCTS[n] for n in ("tb_gemm_desc", "tb_attn_desc", "tb_ff_desc", "tb_chain_desc",
                                                                          "tb_opt_desc"))

_lib = None

IMG_LANCZOS, IMG_BICUBIC = 1, 3
IMG_BILINEAR = 16   # not Pillow's 2: see TB_IMG_BILINEAR


F32_EXACT, F32_SPLIT = 0, 1
_f32_mode = F32_EXACT   # tb_f32_set_mode of EVERY loaded build of the library (and of one loaded later): see set_f32_mode

_half = "fp16"     # the 16-bit float of the ACTIVE library: one process runs one numeric mode (like the reference's accelerator)
_libs = {}


def set_half(kind: str):
    """select the library every `lib()` call returns: "fp16" (libtextboost_hip.so) or "bf16" (libtextboost_hip_bf16.so, same C-ABI, TB_F16 then
    means bfloat16).  Returns the previous kind."""
    global _half, _lib
    assert kind in ("fp16", "bf16"), kind
    prev, _half = _half, kind
    _lib = _libs.get(kind)
    return prev


@contextlib.contextmanager
def use_half(kind: str):
    """run a block on the other build of the library (host-side dispatch only: every op looks `lib()` up when it is called, so this also
    works while a HIP graph is being captured).  The VAE encoder uses it to stay on the fp16 build in a bf16 run (vae.py)."""
    if kind is None:   # "whatever the process runs"
        yield
        return
    prev = set_half(kind)
    try:
        yield
    finally:
        set_half(prev)


def set_f32_mode(mode: int) -> int:
    """how the fp32 contractions multiply (tb_f32_set_mode): 0 = exact fp32 products, 1 = three bf16 products of split operands.  The mode
    is a property of the process, not of one build of the library: it is applied to every build that is loaded (`use_half` switches
    builds around the VAE) and `lib()` applies it to a build it loads later.  Returns the previous mode."""
    global _f32_mode
    mode = int(mode)
    if mode not in (F32_EXACT, F32_SPLIT):
        raise ValueError(f"f32 mode {mode}: 0 (exact) or 1 (split)")
    prev, _f32_mode = _f32_mode, mode
    for h in _libs.values():
        rc = h.tb_f32_set_mode(mode)
        if rc < 0:
            raise RuntimeError(f"tb_f32_set_mode({mode}) failed with code {rc}")
    return prev


def get_f32_mode() -> int:
    return _f32_mode


def half_kind() -> str:
    return _half


def half_dtype():
    """torch dtype of the active library's 16-bit float"""
    return torch.bfloat16 if _half == "bf16" else torch.float16


def lib():
    global _lib
    if _lib is None:
        path = LIB_PATH_BF16 if _half == "bf16" else LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -m textboost_amd.build` (hipcc --offload-arch=gfx950). "
                "textboost_amd has no CPU fallback.")
        _lib = C.CDLL(path)
        for name, (args, res) in _SIGS.items():
            fn = getattr(_lib, name)  # AttributeError here = library older than the header
            fn.argtypes, fn.restype = args, res
        _libs[_half] = _lib
        if _lib.tb_f32_set_mode(_f32_mode) < 0:
            raise RuntimeError(f"tb_f32_set_mode({_f32_mode}) failed")
    return _lib


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        detail = ""
        if rc == -5:
            detail = " (HIP: " + (lib().tb_last_hip_error() or b"?").decode() + ")"
        raise RuntimeError(f"{what} failed with code {rc}{detail}")
