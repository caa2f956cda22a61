"""The verdict of msclip_clip_coef_guarded (include/msclip_ext4.h) restated in torch, for the tests: runs wherever the partials
live, CPU included."""
import torch

EXPONENT = 0x7F800000


def nonfinite_mask(partials):
    """bool mask: the exponent field of the fp32 bit pattern is all ones (NaN, +Inf, -Inf) -- the kernel's test."""
    assert partials.dtype == torch.float32
    return (partials.contiguous().view(torch.int32) & EXPONENT) == EXPONENT


def verdict(partials, total_before=0):
    """-> [skip, total_before + skip, smallest index of a non-finite partial or -1, number of non-finite partials]: what the
    call leaves in state[0..4) when state[1] held total_before."""
    bad = nonfinite_mask(partials)
    count = int(bad.sum())
    skip = int(count > 0)
    first = int(torch.nonzero(bad)[0]) if count else -1
    return [skip, total_before + skip, first, count]


def norm64(partials):
    """sqrt of the sum of the partials in double: what out[0] holds to fp32 rounding (NaN / Inf where the sum is)."""
    return float(torch.sqrt(partials.double().sum()))
