"""The host side of the training augmentation: pure functions, no GPU needed.

* `random_resized_crop_boxes`: torchvision's RandomResizedCrop.get_params for a whole batch from given uniforms -- the boxes that
  msclip_resized_crop (include/msclip_input.h) then cuts and resamples on the device;
* `aug_settings`: what the reference's config says about augmentation (lib/config/default.py:88-107: AUG.SCALE / AUG.RATIO,
  TRAIN.IMAGE_SIZE, INPUT.MEAN / INPUT.STD), and a refusal of every switch this project does not implement;
* `epoch_order`: which samples a rank sees in an epoch, batch by batch.
"""
import math

import torch

DEFAULT_SCALE = (0.08, 1.0)                              # lib/config/default.py:90
DEFAULT_RATIO = (3.0 / 4.0, 4.0 / 3.0)                   # lib/config/default.py:91
ATTEMPTS = 10                                            # torchvision: ten draws, then the centred fallback


def random_resized_crop_boxes(sizes, u, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO):
    """sizes: int [B, 2] (h, w); u: uniforms in [0, 1) of shape [B, 10, 4] -> int32 [B, 4] (top, left, height, width).

    torchvision's RandomResizedCrop.get_params, vectorised, in float64.  Attempt t of image b draws area = H W (s0 + u0 (s1 - s0)),
    ar = exp(log r0 + u1 (log r1 - log r0)), w = round(sqrt(area ar)), h = round(sqrt(area / ar)) (round-half-even) and is accepted
    when 0 < w <= W and 0 < h <= H, with top = floor(u2 (H - h + 1)), left = floor(u3 (W - w + 1)); the first accepted attempt
    wins.  Fallback: the centred box of the whole image with its ratio clamped into `ratio`.  Runs wherever its tensors live."""
    if sizes.dim() != 2 or sizes.shape[1] != 2 or sizes.dtype.is_floating_point:
        raise ValueError(f"sizes: int [B, 2], got {sizes.dtype} {tuple(sizes.shape)}")
    B = sizes.shape[0]
    if tuple(u.shape) != (B, ATTEMPTS, 4) or not u.dtype.is_floating_point:
        raise ValueError(f"u: float [{B}, {ATTEMPTS}, 4], got {u.dtype} {tuple(u.shape)}")
    if not (0.0 < scale[0] <= scale[1]) or not (0.0 < ratio[0] <= ratio[1]):
        raise ValueError(f"scale = {scale!r}, ratio = {ratio!r}: each 0 < low <= high")
    if B and int(sizes.min()) < 1:
        raise ValueError("sizes: every extent must be at least 1")
    u = u.to(torch.float64)
    H, W = sizes[:, 0:1].to(torch.float64), sizes[:, 1:2].to(torch.float64)               # [B, 1]
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    area = (H * W) * (scale[0] + u[:, :, 0] * (scale[1] - scale[0]))                      # [B, 10]
    ar = torch.exp(log_r[0] + u[:, :, 1] * (log_r[1] - log_r[0]))
    w, h = torch.round(torch.sqrt(area * ar)), torch.round(torch.sqrt(area / ar))
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    top, left = torch.floor(u[:, :, 2] * (H - h + 1.0)), torch.floor(u[:, :, 3] * (W - w + 1.0))
    first = ok.to(torch.int8).argmax(dim=1, keepdim=True)                                 # (the first maximum: the first accepted)
    tried = torch.stack([top, left, h, w], dim=2).gather(1, first.unsqueeze(2).expand(B, 1, 4)).squeeze(1)   # [B, 4]
    # the fallback
    H, W = H.squeeze(1), W.squeeze(1)
    in_ratio = W / H
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    fw = torch.where(wide, torch.round(H * max(ratio)), W)
    fh = torch.where(narrow, torch.round(W / min(ratio)), H)
    fallback = torch.stack([torch.floor((H - fh) / 2.0), torch.floor((W - fw) / 2.0), fh, fw], dim=1)
    return torch.where(ok.any(dim=1, keepdim=True), tried, fallback).to(torch.int32)


# every augmentation switch of the reference that this project does not implement: (key, "is it on?")
_UNSUPPORTED = (
    ("AUG.COLOR_JITTER", lambda v: bool(v) and float(list(v)[-1]) > 0.0),      # [b, c, s, h, probability]
    ("AUG.GRAY_SCALE", lambda v: float(v or 0.0) > 0.0),
    ("AUG.GAUSSIAN_BLUR", lambda v: float(v or 0.0) > 0.0),
    ("AUG.MIXUP", lambda v: float(v or 0.0) > 0.0),
    ("AUG.MIXCUT", lambda v: float(v or 0.0) > 0.0),
    ("AUG.MIXCUT_MINMAX", lambda v: bool(v)),
    ("AUG.RANDOM_CENTER_CROP", lambda v: bool(v)),
    ("AUG.TIMM_AUG.USE_LOADER", lambda v: bool(v)),
    ("AUG.TIMM_AUG.USE_TRANSFORM", lambda v: bool(v)),
)
_ABSENT = object()


def _lookup(config, key):
    node = config
    for part in key.split("."):
        if not isinstance(node, dict) or part not in node:
            return _ABSENT
        node = node[part]
    return node


def aug_settings(config):
    """-> dict(scale, ratio, size, interpolation, mean, std, flip_prob) from the config, where present: AUG.SCALE (default
    (0.08, 1.0)), AUG.RATIO ((3/4, 4/3)), TRAIN.IMAGE_SIZE ([224, 224]; a square), INPUT.MEAN / INPUT.STD (ImageNet's), and two
    keys of this project: AUG.INTERPOLATION (a PIL code, 2 bilinear or 3 bicubic; default 3, the eval transform's filter) and
    AUG.FLIP_PROB (default 0.0: captions say "left").  An absent node means the reference's default, every switch off; a switch of
    the reference that is ON and not implemented here raises NotImplementedError naming its key."""
    for key, on in _UNSUPPORTED:
        v = _lookup(config, key)
        if v is not _ABSENT and on(v):
            raise NotImplementedError(f"{key} = {v!r}: this augmentation is not implemented (random-resized crop and horizontal "
                                      "flip are; set the key to its off value)")

    def get(key, default):
        v = _lookup(config, key)
        return default if v is _ABSENT else v
    scale = tuple(float(v) for v in get("AUG.SCALE", DEFAULT_SCALE))
    ratio = tuple(float(v) for v in get("AUG.RATIO", DEFAULT_RATIO))
    size = get("TRAIN.IMAGE_SIZE", [224, 224])
    size = [int(size), int(size)] if isinstance(size, (int, float)) else [int(v) for v in size]
    if len(scale) != 2 or len(ratio) != 2 or not 0.0 < scale[0] <= scale[1] or not 0.0 < ratio[0] <= ratio[1]:
        raise ValueError(f"AUG.SCALE = {scale!r}, AUG.RATIO = {ratio!r}: each a pair 0 < low <= high")
    if len(size) != 2 or size[0] != size[1] or size[0] <= 0:
        raise ValueError(f"TRAIN.IMAGE_SIZE = {size!r}: the model takes square images")
    interpolation = int(get("AUG.INTERPOLATION", 3))
    if interpolation not in (2, 3):
        raise ValueError(f"AUG.INTERPOLATION = {interpolation!r}: PIL's code 2 (bilinear) or 3 (bicubic)")
    flip_prob = float(get("AUG.FLIP_PROB", 0.0))
    if not 0.0 <= flip_prob <= 1.0:
        raise ValueError(f"AUG.FLIP_PROB = {flip_prob!r}: a probability")
    mean = tuple(float(v) for v in get("INPUT.MEAN", (0.485, 0.456, 0.406)))
    std = tuple(float(v) for v in get("INPUT.STD", (0.229, 0.224, 0.225)))
    return dict(scale=scale, ratio=ratio, size=size[0], interpolation=interpolation, mean=mean, std=std, flip_prob=flip_prob)


def epoch_order(n, epoch, seed, rank=0, world=1, batch_size=1):
    """The sample indices of this rank's batches in `epoch`: int64 [batches, batch_size].  One permutation of range(n) per
    (seed, epoch), truncated so that EVERY rank gets the same number of whole batches; rank r takes its indices r::world."""
    if not (0 <= rank < world) or batch_size < 1 or n < 0:
        raise ValueError(f"rank {rank} of {world}, batch_size {batch_size}, n {n}")
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
    perm = torch.randperm(n, generator=g)
    nb = n // (world * batch_size)
    return perm[:nb * world * batch_size][rank::world].reshape(nb, batch_size)
