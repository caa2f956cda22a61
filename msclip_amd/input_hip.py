"""ctypes binding of the training input path of libmsclip_hip.so (the C ABI declared in include/msclip_input.h).

A module of its own beside msclip_amd/hip.py: that module's table of bound headers stays as it is, and this header is versioned on
its own (MSCLIP_INPUT_ABI_VERSION).  The same rules hold: the header is read with abi.load, restype / argtypes come from the parsed
prototypes, a library of another version is refused, and there is no CPU or eager-PyTorch fallback.
"""
import ctypes
import os
import re

import torch

from . import abi, hip

HEADER = os.path.join(os.path.dirname(abi.HEADER), "msclip_input.h")
VERSION_MACRO = "MSCLIP_INPUT_ABI_VERSION"
_INPUT = abi.load(HEADER, VERSION_MACRO)
INPUT_ABI_VERSION = _INPUT.version
INPUT_EXPORTS = tuple(_INPUT.protos)
with open(HEADER) as _f:
    _TEXT = _f.read()
CROP_MAX_SCALE = int(re.search(r"^#define MSCLIP_CROP_MAX_SCALE (\d+)$", _TEXT, re.M).group(1))
CROP_LDS_BYTES = int(re.search(r"^#define MSCLIP_CROP_LDS_BYTES (\d+)$", _TEXT, re.M).group(1))
FILTERS = (2, 3)                                         # PIL's codes: bilinear, bicubic

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(hip.LIB_PATH):
            raise hip.HipUnavailable(f"{hip.LIB_PATH} is missing: run msclip_amd/csrc/build.sh (no CPU fallback exists)")
        L = ctypes.CDLL(hip.LIB_PATH)
        for name, (restype, argtypes) in _INPUT.protos.items():
            fn = getattr(L, name, None)
            if fn is None:
                raise hip.HipUnavailable(f"{hip.LIB_PATH} does not export {name}, which include/msclip_input.h declares: rebuild "
                                         "(bash msclip_amd/csrc/build.sh)")
            fn.restype, fn.argtypes = restype, argtypes
        have = L.msclip_input_abi_version()
        if have != INPUT_ABI_VERSION:
            raise hip.HipUnavailable(f"{hip.LIB_PATH} has input ABI version {have}, this binding needs {INPUT_ABI_VERSION}: rebuild "
                                     "(bash msclip_amd/csrc/build.sh)")
        _lib = L
    return _lib


def crop_band(slot_h, slot_w, out_h, out_w, filter=3):
    """Output rows of a workgroup of msclip_resized_crop for these extents (-1: the call would be rejected)."""
    return lib().msclip_resized_crop_band(slot_h, slot_w, out_h, out_w, filter)


def crop_lds(slot_h, slot_w, out_h, out_w, filter=3):
    return lib().msclip_resized_crop_lds(slot_h, slot_w, out_h, out_w, filter)


def _i32(t, shape, what):
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
        raise ValueError(f"resized_crop: {what} must be a contiguous int32 device tensor of shape {list(shape)}, got "
                         f"{t.dtype} {list(t.shape)} on {t.device}")


def resized_crop(src, dims, boxes, lut, size, *, flip=None, filter=3, bf16=False, out=None, want_u8=False):
    """PIL's crop(box).resize(size, filter) + flip + per-channel table look-up of a staged batch, on the current stream.

    src uint8 [B, slot_h, slot_w, 3]; dims int32 [B, 2] (h, w); boxes int32 [B, 4] (top, left, height, width); flip int32 [B] or
    None; lut fp32 [3, 256] (zeroshot.normalise_lut); size = S or (out_h, out_w).  All on one device.
    -> out [B, 3, out_h, out_w] fp32 (bf16=True: bfloat16), or (out, out_u8 uint8 [B, out_h, out_w, 3]) with want_u8."""
    hip.require_gpu()
    out_h, out_w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_cuda or not src.is_contiguous():
        raise ValueError(f"resized_crop: src must be a contiguous uint8 device tensor [B, slot_h, slot_w, 3], got {src.dtype} "
                         f"{list(src.shape)} on {src.device}")
    B, slot_h, slot_w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    _i32(dims, (B, 2), "dims")
    _i32(boxes, (B, 4), "boxes")
    if flip is not None:
        _i32(flip, (B,), "flip")
    if lut.dtype != torch.float32 or not lut.is_cuda or not lut.is_contiguous() or lut.numel() != 768:
        raise ValueError("resized_crop: lut must be a contiguous fp32 device tensor of 3 x 256 values")
    if filter not in FILTERS:
        raise ValueError(f"resized_crop: filter {filter!r} is not one of PIL's codes 2 (bilinear), 3 (bicubic)")
    if any(t is not None and t.device != src.device for t in (dims, boxes, flip, lut, out)):
        raise ValueError("resized_crop: all tensors must live on src's device")
    if B == 0 or out_h <= 0 or out_w <= 0:
        raise ValueError(f"resized_crop: empty batch or output ({B} samples, {out_h} x {out_w})")
    if slot_h > CROP_MAX_SCALE * out_h or slot_w > CROP_MAX_SCALE * out_w:
        raise ValueError(f"resized_crop: slots of {slot_h} x {slot_w} are more than {CROP_MAX_SCALE} times the output "
                         f"{out_h} x {out_w} (MSCLIP_CROP_MAX_SCALE)")
    L = lib()
    if L.msclip_resized_crop_band(slot_h, slot_w, out_h, out_w, filter) < 0:
        raise ValueError(f"resized_crop: {slot_h} x {slot_w} -> {out_h} x {out_w} does not fit the LDS budget of "
                         f"{CROP_LDS_BYTES} bytes (include/msclip_input.h)")
    dtype = torch.bfloat16 if bf16 else torch.float32
    if out is None:
        out = torch.empty(B, 3, out_h, out_w, dtype=dtype, device=src.device)
    elif out.dtype != dtype or tuple(out.shape) != (B, 3, out_h, out_w) or not out.is_contiguous():
        raise ValueError(f"resized_crop: out must be a contiguous {dtype} tensor [{B}, 3, {out_h}, {out_w}]")
    u8 = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=src.device) if want_u8 else None
    with torch.cuda.device(src.device):
        hip._check(L.msclip_resized_crop(hip._p(src), slot_h, slot_w, hip._p(dims), hip._p(boxes), hip._p(flip), hip._p(lut), B,
                                         filter, out_h, out_w, hip._p(out), int(bf16), hip._p(u8), hip._stream()),
                   "msclip_resized_crop")
    return (out, u8) if want_u8 else out
