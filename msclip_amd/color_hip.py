"""ctypes binding of the colour stage of the training input path of libmsclip_hip.so (the C ABI declared in include/msclip_color.h).

A module of its own beside msclip_amd/hip.py and msclip_amd/input_hip.py: their tables of bound headers stay as they are, and this
header is versioned on its own (MSCLIP_COLOR_ABI_VERSION).  The same rules hold: the header is read with abi.load, restype /
argtypes come from the parsed prototypes, a library of another version is refused, and there is no CPU or eager-PyTorch fallback.
"""
import ctypes
import os
import re

import torch

from . import abi, hip

HEADER = os.path.join(os.path.dirname(abi.HEADER), "msclip_color.h")
VERSION_MACRO = "MSCLIP_COLOR_ABI_VERSION"
_COLOR = abi.load(HEADER, VERSION_MACRO)
COLOR_ABI_VERSION = _COLOR.version
COLOR_EXPORTS = tuple(_COLOR.protos)
with open(HEADER) as _f:
    _TEXT = _f.read()
COLOR_RADIUS = int(re.search(r"^#define MSCLIP_COLOR_RADIUS (\d+)$", _TEXT, re.M).group(1))
COLOR_LDS_BYTES = int(re.search(r"^#define MSCLIP_COLOR_LDS_BYTES (\d+)$", _TEXT, re.M).group(1))
JITTER, GRAY, BLUR = 1, 2, 4                             # the bits of `stages`
OPS, COEF = 8, 12                                        # entries per image of `ops` and `coef`

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(hip.LIB_PATH):
            raise hip.HipUnavailable(f"{hip.LIB_PATH} is missing: run msclip_amd/csrc/build.sh (no CPU fallback exists)")
        L = ctypes.CDLL(hip.LIB_PATH)
        for name, (restype, argtypes) in _COLOR.protos.items():
            fn = getattr(L, name, None)
            if fn is None:
                raise hip.HipUnavailable(f"{hip.LIB_PATH} does not export {name}, which include/msclip_color.h declares: rebuild "
                                         "(bash msclip_amd/csrc/build.sh)")
            fn.restype, fn.argtypes = restype, argtypes
        have = L.msclip_color_abi_version()
        if have != COLOR_ABI_VERSION:
            raise hip.HipUnavailable(f"{hip.LIB_PATH} has colour ABI version {have}, this binding needs {COLOR_ABI_VERSION}: rebuild "
                                     "(bash msclip_amd/csrc/build.sh)")
        _lib = L
    return _lib


def augment_band(H, W):
    """Rows of a workgroup of msclip_color_augment for these extents (-1: the call would be rejected)."""
    return lib().msclip_color_augment_band(H, W)


def augment_lds(H, W):
    return lib().msclip_color_augment_lds(H, W)


def color_augment(src_u8, ops, coef, lut, *, stages, bf16=False, out=None, want_u8=False):
    """Colour jitter, grayscale, Gaussian blur and the per-channel table look-up of a batch, on the current stream.

    src_u8 uint8 [B, H, W, 3] (resized_crop's out_u8); ops int32 [B, 8] and coef fp32 [B, 12] (augment.colour_params); lut fp32
    [3, 256]; stages: a mask of JITTER | GRAY | BLUR, what the launch provides for (the per-image entries of ops decide per image).
    All on one device.  -> out [B, 3, H, W] fp32 (bf16=True: bfloat16), or (out, out_u8 uint8 [B, H, W, 3]) with want_u8."""
    hip.require_gpu()
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_cuda or not src_u8.is_contiguous():
        raise ValueError(f"color_augment: src_u8 must be a contiguous uint8 device tensor [B, H, W, 3], got {src_u8.dtype} "
                         f"{list(src_u8.shape)} on {src_u8.device}")
    B, H, W = int(src_u8.shape[0]), int(src_u8.shape[1]), int(src_u8.shape[2])
    for t, dtype, shape, what in ((ops, torch.int32, (B, OPS), "ops"), (coef, torch.float32, (B, COEF), "coef")):
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"color_augment: {what} must be a contiguous {dtype} device tensor of shape {list(shape)}, got "
                             f"{t.dtype} {list(t.shape)} on {t.device}")
    if lut.dtype != torch.float32 or not lut.is_cuda or not lut.is_contiguous() or lut.numel() != 768:
        raise ValueError("color_augment: lut must be a contiguous fp32 device tensor of 3 x 256 values")
    if isinstance(stages, bool) or not isinstance(stages, int) or not 0 <= stages <= 7:
        raise ValueError(f"color_augment: stages = {stages!r} is not a mask of JITTER (1), GRAY (2), BLUR (4)")
    if any(t is not None and t.device != src_u8.device for t in (ops, coef, lut, out)):
        raise ValueError("color_augment: all tensors must live on src_u8's device")
    if B == 0 or H == 0 or W == 0:
        raise ValueError(f"color_augment: empty batch or image ({B} samples, {H} x {W})")
    L = lib()
    if L.msclip_color_augment_band(H, W) < 0:
        raise ValueError(f"color_augment: a row of {W} pixels does not fit the LDS budget of {COLOR_LDS_BYTES} bytes "
                         "(include/msclip_color.h)")
    dtype = torch.bfloat16 if bf16 else torch.float32
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=dtype, device=src_u8.device)
    elif out.dtype != dtype or tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous():
        raise ValueError(f"color_augment: out must be a contiguous {dtype} tensor [{B}, 3, {H}, {W}]")
    u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=src_u8.device) if want_u8 else None
    work = torch.empty(B, dtype=torch.int32, device=src_u8.device) if stages & JITTER else None
    with torch.cuda.device(src_u8.device):
        hip._check(L.msclip_color_augment(hip._p(src_u8), hip._p(ops), hip._p(coef), hip._p(lut), B, H, W, stages, hip._p(work),
                                          hip._p(out), int(bf16), hip._p(u8), hip._stream()), "msclip_color_augment")
    return (out, u8) if want_u8 else out
