"""The host side of the training augmentation: pure functions, no GPU needed.

* `random_resized_crop_boxes`: torchvision's RandomResizedCrop.get_params for a whole batch from given uniforms -- the boxes that
  msclip_resized_crop (include/msclip_input.h) then cuts and resamples on the device;
* `aug_settings`: what the reference's config says about augmentation (lib/config/default.py:88-107: AUG.SCALE / AUG.RATIO,
  TRAIN.IMAGE_SIZE, INPUT.MEAN / INPUT.STD; with colour=True also AUG.COLOR_JITTER / AUG.GRAY_SCALE / AUG.GAUSSIAN_BLUR), and a
  refusal of every switch this project does not implement;
* `colour_params`, `blur_weights`, `colour_stages`: the per-image records, the blur weights and the stage mask that
  msclip_color_augment (include/msclip_color.h) takes, from given uniforms;
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


_COLOUR_KEYS = ("AUG.COLOR_JITTER", "AUG.GRAY_SCALE", "AUG.GAUSSIAN_BLUR")


def _colour_settings(config):
    """The three colour keys, validated -> dict(color_jitter=(b, c, s, h, p), gray_scale=p, gaussian_blur=p)."""
    cj = _lookup(config, "AUG.COLOR_JITTER")
    cj = (0.0, 0.0, 0.0, 0.0, 0.0) if cj is _ABSENT or not cj else tuple(float(v) for v in cj)
    if len(cj) != 5 or any(not math.isfinite(v) for v in cj) or min(cj[:4]) < 0.0 or cj[3] > 0.5 or not 0.0 <= cj[4] <= 1.0:
        raise ValueError(f"AUG.COLOR_JITTER = {cj!r}: [brightness, contrast, saturation, hue, probability] with strengths >= 0, "
                         "hue <= 0.5 and a probability in [0, 1]")
    out = {"color_jitter": cj}
    for key, name in (("AUG.GRAY_SCALE", "gray_scale"), ("AUG.GAUSSIAN_BLUR", "gaussian_blur")):
        v = _lookup(config, key)
        p = 0.0 if v is _ABSENT or v is None else float(v)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"{key} = {p!r}: a probability")
        out[name] = p
    return out


def aug_settings(config, colour=False):
    """-> dict(scale, ratio, size, interpolation, mean, std, flip_prob) from the config, where present: AUG.SCALE (default
    (0.08, 1.0)), AUG.RATIO ((3/4, 4/3)), TRAIN.IMAGE_SIZE ([224, 224]; a square), INPUT.MEAN / INPUT.STD (ImageNet's), and two
    keys of this project: AUG.INTERPOLATION (a PIL code, 2 bilinear or 3 bicubic; default 3, the eval transform's filter) and
    AUG.FLIP_PROB (default 0.0: captions say "left").  An absent node means the reference's default, every switch off; a switch of
    the reference that is ON and not implemented here raises NotImplementedError naming its key.
    colour=True (callers that run the colour stage, msclip_color_augment): AUG.COLOR_JITTER, AUG.GRAY_SCALE and AUG.GAUSSIAN_BLUR
    are accepted and validated instead of refused, and the dict gains color_jitter = (b, c, s, h, p), gray_scale = p and
    gaussian_blur = p."""
    for key, on in _UNSUPPORTED:
        if colour and key in _COLOUR_KEYS:
            continue
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
    out = dict(scale=scale, ratio=ratio, size=size[0], interpolation=interpolation, mean=mean, std=std, flip_prob=flip_prob)
    if colour:
        out.update(_colour_settings(config))
    return out


# ---- the colour stage: what msclip_color_augment (include/msclip_color.h) is told per image
BLUR_RADIUS = 6                                          # MSCLIP_COLOR_RADIUS: ceil(3 sigma) at the largest sigma
SIGMA = (0.1, 2.0)                                       # the reference's GaussianBlur
COLOUR_DRAWS = 9                                         # uniforms per image of colour_params
_ORDERS = None


def _orders():
    global _ORDERS
    if _ORDERS is None:
        import itertools
        _ORDERS = torch.tensor(list(itertools.permutations(range(4))), dtype=torch.int32)       # lexicographic, [24, 4]
    return _ORDERS


def colour_stages(settings):
    """The `stages` mask of msclip_color_augment for these settings: jitter 1, gray 2, blur 4; 0: the colour stage is off."""
    cj = settings.get("color_jitter", (0.0,) * 5)
    return ((1 if cj[4] > 0.0 and max(cj[:4]) > 0.0 else 0) | (2 if settings.get("gray_scale", 0.0) > 0.0 else 0)
            | (4 if settings.get("gaussian_blur", 0.0) > 0.0 else 0))


def blur_weights(sigma):
    """sigma [..] -> fp32 [.., 7]: w_k = exp(-k^2 / 2 sigma^2) / (w_0 + 2 sum_{k >= 1} w_k), k = 0 ... 6, computed in fp64 and
    rounded once."""
    sigma = torch.as_tensor(sigma, dtype=torch.float64)
    k = torch.arange(BLUR_RADIUS + 1, dtype=torch.float64)
    w = torch.exp(-(k * k) / (2.0 * sigma.unsqueeze(-1) ** 2))
    return (w / (w[..., :1] + 2.0 * w[..., 1:].sum(dim=-1, keepdim=True))).to(torch.float32)


def colour_params(u, settings):
    """u: uniforms in [0, 1) of shape [B, 9]; settings: aug_settings(config, colour=True)
    -> (ops int32 [B, 8], coef fp32 [B, 12]), the per-image records of msclip_color_augment.  A pure function, in float64.

    With torchvision's semantics (RandomApply([ColorJitter(b, c, s, h)], p), RandomGrayscale(p), RandomApply([GaussianBlur], p)):
    u0 < p applies the jitter; floor(24 u1) picks its op order among the lexicographic permutations of (0 brightness, 1 contrast,
    2 saturation, 3 hue); u2, u3, u4 give f_b, f_c, f_s uniform in [max(0, 1 - x), 1 + x]; u5 gives f_h uniform in [-h, h] and the
    shift int(255 f_h) & 255 (truncation toward zero); u6 < p turns the image gray; u7 < p blurs it with sigma = 0.1 + 1.9 u8.
    An op whose strength is 0 is left out of the order (-1).  ops: order[0..3], shift, gray flag, blur flag, 0; coef: f_b, f_c,
    f_s, 0, w0 ... w6, 0.  An image with nothing on gets the all-skip record: order -1, flags 0, factors 1, weights (1, 0 ...)."""
    if u.dim() != 2 or u.shape[1] != COLOUR_DRAWS or not u.dtype.is_floating_point:
        raise ValueError(f"u: float [B, {COLOUR_DRAWS}], got {u.dtype} {tuple(u.shape)}")
    u = u.to(torch.float64)
    B = u.shape[0]
    b, c, s, h, p = (float(v) for v in settings.get("color_jitter", (0.0,) * 5))
    jit = u[:, 0] < p
    order = _orders()[torch.clamp(torch.floor(u[:, 1] * 24.0).to(torch.int64), 0, 23)].clone()
    for op, strength in enumerate((b, c, s, h)):
        if strength == 0.0:
            order[order == op] = -1
    order[~jit] = -1
    ops = torch.zeros(B, 8, dtype=torch.int32)
    coef = torch.zeros(B, 12, dtype=torch.float32)
    ops[:, :4] = order
    for col, x in enumerate((b, c, s)):
        lo, hi = max(0.0, 1.0 - x), 1.0 + x
        f = lo + u[:, 2 + col] * (hi - lo)
        coef[:, col] = torch.where(jit, f, torch.ones_like(f)).to(torch.float32)
    shift = torch.trunc((-h + u[:, 5] * (2.0 * h)) * 255.0).to(torch.int64) & 255
    ops[:, 4] = torch.where(jit & (h > 0.0), shift, torch.zeros_like(shift)).to(torch.int32)
    ops[:, 5] = (u[:, 6] < float(settings.get("gray_scale", 0.0))).to(torch.int32)
    blur = u[:, 7] < float(settings.get("gaussian_blur", 0.0))
    ops[:, 6] = blur.to(torch.int32)
    w = blur_weights(SIGMA[0] + u[:, 8] * (SIGMA[1] - SIGMA[0]))
    skip = torch.zeros(BLUR_RADIUS + 1, dtype=torch.float32)
    skip[0] = 1.0
    coef[:, 4:11] = torch.where(blur.unsqueeze(1), w, skip.unsqueeze(0))
    return ops, coef


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
