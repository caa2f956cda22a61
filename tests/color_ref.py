"""The arithmetic of include/msclip_color.h restated in numpy, independent of msclip_amd: fp32 / fp64 exactly as the header writes it
and in the same summation order.  Every function maps uint8 [H, W, 3] to uint8 [H, W, 3] unless it says otherwise.

`augment(src, ops, coef, lut, stages)` is the whole of msclip_color_augment for a batch, the device-side guards included; the `pil_*`
functions are what PIL computes for the same step (the oracle: torchvision's ColorJitter / RandomGrayscale on PIL images call these).
"""
import itertools

import numpy as np

F = np.float32
ORDERS = list(itertools.permutations(range(4)))          # lexicographic: augment.colour_params' order index
RADIUS = 6


def gray_value(img):
    """-> int32 [H, W]"""
    x = img.astype(np.int32)
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 32768) >> 16


def blend(d, x, f):
    """d, x integer arrays (broadcast), f a float -> uint8: t = d + f * (x - d) in fp32 with two roundings."""
    d, x = np.asarray(d, np.int32), np.asarray(x, np.int32)
    prod = (F(f) * (x - d).astype(F)).astype(F)
    t = (d.astype(F) + prod).astype(F)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def brightness(img, f):
    return blend(0, img, f)


def saturation(img, f):
    return blend(gray_value(img)[..., None], img, f)


def contrast_mean(img):
    return int(np.floor(float(gray_value(img).astype(np.int64).sum()) / (float(img.shape[0]) * float(img.shape[1])) + 0.5))


def contrast(img, f):
    return blend(contrast_mean(img), img, f)


def rgb_to_hsv(img):
    x = img.astype(np.int32)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(axis=-1), x.min(axis=-1)
    flat = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F)
        s = (cr / maxc.astype(F)).astype(F)
        rc, gc, bc = ((maxc - c).astype(F) / cr for c in (r, g, b))
        rc, gc, bc = rc.astype(F), gc.astype(F), bc.astype(F)
        h_r = (bc - gc).astype(F)
        h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F)
        h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F)
        hh = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b)).astype(F)
        hh = np.fmod(hh.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F)
        hh = np.where(flat, F(0), hh)
        s = np.where(flat, F(0), s)
        h8 = np.clip((hh.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        s8 = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(flat, 0, h8), np.where(flat, 0, s8), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s8, v = (hsv[..., i].astype(np.int32) for i in range(3))
    fh = ((h.astype(F) * F(6)).astype(F) / F(255)).astype(F)
    fs = (s8.astype(F) / F(255)).astype(F)
    fi = np.floor(fh).astype(F)
    f = (fh - fi).astype(F)
    fv = v.astype(F)
    one = F(1)

    def r8(x):
        return np.clip(np.floor(x.astype(np.float64) + 0.5), 0, 255).astype(np.int32)
    p = r8((fv * (one - fs).astype(F)).astype(F))
    q = r8((fv * (one - (fs * f).astype(F)).astype(F)).astype(F))
    t = r8((fv * (one - (fs * (one - f).astype(F)).astype(F)).astype(F)).astype(F))
    i = fi.astype(np.int32) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape, np.int32)
    for k, rgb in enumerate(table):
        for ch in range(3):
            out[..., ch] = np.where(i == k, rgb[ch], out[..., ch])
    out = np.where((s8 == 0)[..., None], v[..., None], out)
    return out.astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + (int(shift) & 255)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def grayscale(img):
    return np.repeat(gray_value(img)[..., None], 3, axis=-1).astype(np.uint8)


def mirror(j, n):
    j = np.asarray(j)
    if n == 1:
        return np.zeros_like(j)
    m = 2 * (n - 1)
    j = ((j % m) + m) % m
    return np.where(j >= n, m - j, j)


def _round_u8(acc):
    r = np.floor(acc + F(0.5))
    with np.errstate(invalid="ignore"):
        return np.where(r > 0, np.minimum(r, 255), 0).astype(np.uint8)       # (not a number: 0)


def _pass(x, w, axis):
    n = x.shape[axis]
    acc = np.zeros(x.shape, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-RADIUS, RADIUS + 1):                 # ascending k, fp32, multiply and add rounded separately
            tap = np.take(x, mirror(np.arange(n) + k, n), axis=axis).astype(F)
            acc = (acc + (F(w[abs(k)]) * tap).astype(F)).astype(F)
    return _round_u8(acc)


def blur(img, w):
    """w: the seven fp32 weights.  Horizontal pass first, uint8 between the passes."""
    w = np.asarray(w, F)
    return _pass(_pass(img, w, 1), w, 0)


def jitter(img, order, factors, shift):
    """order: up to four op codes (0 brightness, 1 contrast, 2 saturation, 3 hue; others skipped), applied left to right."""
    for op in order:
        if op == 0:
            img = brightness(img, factors[0])
        elif op == 1:
            img = contrast(img, factors[1])
        elif op == 2:
            img = saturation(img, factors[2])
        elif op == 3:
            img = hue(img, shift)
    return img


def _guard(f):
    f = F(f)
    if not np.isfinite(f):
        f = F(1)
    return F(min(max(f, F(0)), F(4)))


def augment_u8(src, ops, coef, stages=7):
    """msclip_color_augment's out_u8: src uint8 [B, H, W, 3], ops int [B, 8], coef fp32 [B, 12], with the device-side guards."""
    out = np.empty_like(src)
    for b in range(src.shape[0]):
        img = src[b]
        if stages & 1:
            order, seen = [], set()
            for op in (int(v) for v in ops[b, :4]):
                if 0 <= op <= 3 and op not in seen:
                    seen.add(op)
                    order.append(op)
            img = jitter(img, order, [_guard(f) for f in coef[b, :3]], int(ops[b, 4]) & 255)
        if stages & 2 and ops[b, 5] != 0:
            img = grayscale(img)
        if stages & 4 and ops[b, 6] != 0:
            w = np.asarray(coef[b, 4:11], F)
            img = blur(img, np.where(np.isfinite(w), w, F(0)))
        out[b] = img
    return out


def lookup(u8, lut):
    """uint8 [B, H, W, 3], lut fp32 [3, 256] -> fp32 [B, 3, H, W]"""
    return np.stack([lut[c][u8[..., c]] for c in range(3)], axis=1)


def weights(sigma):
    k = np.arange(RADIUS + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(F)


# ---- what PIL computes
def pil_enhance(img, op, f):
    from PIL import Image, ImageEnhance
    cls = {0: ImageEnhance.Brightness, 1: ImageEnhance.Contrast, 2: ImageEnhance.Color}[op]
    return np.asarray(cls(Image.fromarray(img)).enhance(f), dtype=np.uint8)


def pil_hue(img, shift):
    """torchvision's adjust_hue on a PIL image: the H channel of convert("HSV") plus uint8(shift), wrapped."""
    from PIL import Image
    h, s, v = Image.fromarray(img).convert("HSV").split()
    nh = (np.asarray(h, dtype=np.uint8).astype(np.int32) + (int(shift) & 255)) & 255
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB"), dtype=np.uint8)


def pil_gray(img):
    from PIL import Image
    return np.repeat(np.asarray(Image.fromarray(img).convert("L"), dtype=np.uint8)[..., None], 3, axis=-1)


def pil_jitter(img, order, factors, shift):
    for op in order:
        img = pil_hue(img, shift) if op == 3 else pil_enhance(img, op, float(factors[op]))
    return img


def scipy_blur(img, sigma):
    """The fp64 mirror correlation with the same weights' formula and the same uint8 rounding between the passes."""
    from scipy.ndimage import correlate1d
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    w /= w.sum()
    hor = np.clip(np.floor(correlate1d(img.astype(np.float64), w, axis=1, mode="mirror") + 0.5), 0, 255)
    return np.clip(np.floor(correlate1d(hor, w, axis=0, mode="mirror") + 0.5), 0, 255).astype(np.uint8)


# ---- shared inputs of the host-build test and the GPU test
def make_image(h, w, seed, kind="noise"):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "low":
        return (x // 8 + 100).astype(np.uint8)
    if kind == "gray":
        return np.repeat(x[..., :1], 3, axis=-1)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        return np.clip(np.stack([127.5 + 100 * np.sin(0.11 * (c + 1) * yy + 0.07 * xx + c) for c in range(3)], -1)
                       + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)
    return x


def batch6(h, w, seed=0):
    """Six images that mix every flag combination, contrast first / in the middle / last, and the guards
    -> src uint8 [6, h, w, 3], ops int32 [6, 8], coef fp32 [6, 12]."""
    kinds = ("noise", "smooth", "low", "gray", "noise", "smooth")
    src = np.stack([make_image(h, w, seed * 10 + i, k) for i, k in enumerate(kinds)])
    nan, inf = float("nan"), float("inf")
    ops = np.array([
        [1, 0, 2, 3, 26, 0, 1, 0],                        # contrast first; blur
        [0, 3, 1, 2, 231, 1, 0, 0],                       # contrast in the middle; gray
        [2, 3, 0, 1, 13, 1, 1, 0],                        # contrast last; gray and blur
        [-1, -1, -1, -1, 0, 0, 0, 0],                     # all off
        [7, 1, 1, -9, 256 + 40, 5, -2, 99],               # guards: codes out of range, contrast twice, shift beyond 255, flags "not 0"
        [3, 2, -1, 0, -30, 0, 1, 0],                      # no contrast; a negative shift; NaN / Inf factors below
    ], np.int32)
    coef = np.zeros((6, 12), np.float32)
    coef[:, :3] = [[0.83, 1.4, 0.6], [1.17, 0.6, 2.0], [1.4, 1.17, 0.0], [1.0, 1.0, 1.0], [9.0, -3.0, nan], [inf, 1.0, -inf]]
    for i, sigma in enumerate((2.0, 0.7, 1.3, 0.1, 0.4, 1.9)):
        coef[i, 4:11] = weights(sigma)
    return src, ops, coef
