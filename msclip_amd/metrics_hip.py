"""ctypes binding of the ranking counts of libmsclip_hip.so (the C ABI declared in include/msclip_metrics.h).

A module of its own beside msclip_amd/hip.py, msclip_amd/input_hip.py and msclip_amd/color_hip.py: their tables of bound headers stay
as they are, and this header is versioned on its own (MSCLIP_METRICS_ABI_VERSION).  The same rules hold: the header is read with
abi.load, restype / argtypes come from the parsed prototypes, a library of another version is refused, and there is no CPU or
eager-PyTorch fallback.
"""
import ctypes
import os
import re

import torch

from . import abi, hip

HEADER = os.path.join(os.path.dirname(abi.HEADER), "msclip_metrics.h")
VERSION_MACRO = "MSCLIP_METRICS_ABI_VERSION"
_METRICS = abi.load(HEADER, VERSION_MACRO)
METRICS_ABI_VERSION = _METRICS.version
METRICS_EXPORTS = tuple(_METRICS.protos)
with open(HEADER) as _f:
    _TEXT = _f.read()
RANK_ROWS = int(re.search(r"^#define MSCLIP_RANK_ROWS (\d+)$", _TEXT, re.M).group(1))
RANK_STAGE = int(re.search(r"^#define MSCLIP_RANK_STAGE (\d+)$", _TEXT, re.M).group(1))
MAX_PAIRS = 1 << int(re.search(r"^#define MSCLIP_RANK_LOG2_MAX_PAIRS (\d+)$", _TEXT, re.M).group(1))    # of one call
LAUNCH_PAIRS = 1 << 40                                   # of one launch: rank_counts splits the class range (a shared machine)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(hip.LIB_PATH):
            raise hip.HipUnavailable(f"{hip.LIB_PATH} is missing: run msclip_amd/csrc/build.sh (no CPU fallback exists)")
        L = ctypes.CDLL(hip.LIB_PATH)
        for name, (restype, argtypes) in _METRICS.protos.items():
            fn = getattr(L, name, None)
            if fn is None:
                raise hip.HipUnavailable(f"{hip.LIB_PATH} does not export {name}, which include/msclip_metrics.h declares: rebuild "
                                         "(bash msclip_amd/csrc/build.sh)")
            fn.restype, fn.argtypes = restype, argtypes
        have = L.msclip_metrics_abi_version()
        if have != METRICS_ABI_VERSION:
            raise hip.HipUnavailable(f"{hip.LIB_PATH} has metrics ABI version {have}, this binding needs {METRICS_ABI_VERSION}: "
                                     "rebuild (bash msclip_amd/csrc/build.sh)")
        _lib = L
    return _lib


def class_chunks(N, C):
    """[(c0, cols)]: the class range [0, C) cut so that a launch compares at most LAUNCH_PAIRS pairs (N * N * cols)."""
    if N * N > LAUNCH_PAIRS:
        raise ValueError(f"rank_counts: {N} samples are {N * N} comparisons per class, over the {LAUNCH_PAIRS} of one launch")
    per = max(1, LAUNCH_PAIRS // (N * N))
    return [(c0, min(per, C - c0)) for c0 in range(0, C, per)]


def rank_counts(S, Y, *, want_gt=True, out=None):
    """msclip_rank_counts over every column of S, on the current stream.

    S fp32 [N, C] and Y uint8 [N, C] (not 0 = positive) on one device; a column window of a wider matrix is fine (stride(1) == 1).
    -> (ge_pos, ge_neg, gt_neg, npos, nbad): int32 [C, N] x 3 (gt_neg None without want_gt) and int32 [C] x 2, as the header states
    them.  out: a tuple of such tensors to write into (rows may be longer than N: the slack is not touched; its gt_neg is
    ignored without want_gt)."""
    hip.require_gpu()
    for t, dt, what in ((S, torch.float32, "S"), (Y, torch.uint8, "Y")):
        if t.dtype != dt or t.dim() != 2 or not t.is_cuda or t.stride(1) != 1:
            raise ValueError(f"rank_counts: {what} must be a {dt} device matrix with unit column stride, got {t.dtype} "
                             f"{list(t.shape)} strides {t.stride()} on {t.device}")
    if S.shape != Y.shape or S.device != Y.device:
        raise ValueError(f"rank_counts: S {list(S.shape)} on {S.device} and Y {list(Y.shape)} on {Y.device} do not match")
    N, C = int(S.shape[0]), int(S.shape[1])
    if N < 1 or C < 1:
        raise ValueError(f"rank_counts: empty set ({N} samples, {C} classes)")
    chunks = class_chunks(N, C)                           # (every chunk is under the entry point's own bound, MAX_PAIRS)
    lds = S.stride(0) if N > 1 else max(C, S.stride(0))
    ldy = Y.stride(0) if N > 1 else max(C, Y.stride(0))
    if out is None:
        ge_pos, ge_neg = (torch.empty(C, N, dtype=torch.int32, device=S.device) for _ in range(2))
        gt_neg = torch.empty(C, N, dtype=torch.int32, device=S.device) if want_gt else None
        npos, nbad = (torch.empty(C, dtype=torch.int32, device=S.device) for _ in range(2))
    else:
        ge_pos, ge_neg, gt_neg, npos, nbad = out
        if not want_gt:
            gt_neg = None                                    # (not stored, whatever the tuple carries)
        for t in (ge_pos, ge_neg, gt_neg):
            if t is not None and (t.dtype != torch.int32 or t.device != S.device or t.dim() != 2 or t.shape[0] < C or t.shape[1] < N
                                  or t.stride(1) != 1 or t.stride(0) != ge_pos.stride(0)):
                raise ValueError("rank_counts: out counts must be int32 [>= C, >= N] device matrices of one row stride")
        for t in (npos, nbad):
            if t.dtype != torch.int32 or t.device != S.device or t.dim() != 1 or t.numel() < C or not t.is_contiguous():
                raise ValueError("rank_counts: out totals must be contiguous int32 [>= C] device vectors")
    ldn = ge_pos.stride(0) if C > 1 or ge_pos.shape[0] > 1 else max(N, ge_pos.stride(0))
    L = lib()
    with torch.cuda.device(S.device):
        for c0, cols in chunks:
            hip._check(L.msclip_rank_counts(hip._p(S[:, c0:]), lds, hip._p(Y[:, c0:]), ldy, N, cols, hip._p(ge_pos[c0:]),
                                            hip._p(ge_neg[c0:]), hip._p(gt_neg[c0:]) if gt_neg is not None else None, ldn,
                                            hip._p(npos[c0:]), hip._p(nbad[c0:]), hip._stream()), "msclip_rank_counts")
    return ge_pos, ge_neg, gt_neg, npos, nbad
