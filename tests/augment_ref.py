"""Reference statements for the training input path, independent of msclip_amd (numpy + PIL only):

* `resized_crop`: the resampling of include/msclip_input.h in fp64 numpy -- per axis the taps of PIL's antialiased resize restricted
  to the crop box, horizontal pass first, the result rounded and clamped to uint8 before the vertical pass (`single_pass=True`
  drops that intermediate rounding: what the arithmetic would be without it);
* `get_params`: torchvision's RandomResizedCrop.get_params as a loop over ten attempts, fed with given uniforms;
* `make_files`: small JPEG / PNG files of mixed sizes and modes.
"""
import math
import os

import numpy as np


def _filter(code, x):
    x = np.abs(x)
    if code == 2:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def axis_matrix(n, m, code, dtype=np.float64):
    """[m, n] weights of one axis: box extent n -> output extent m (`dtype` float32: the same formulas in fp32)."""
    f = dtype
    scale = f(n) / f(m)
    fs = max(scale, f(1.0))
    sup = f(1.0 if code == 2 else 2.0) * fs
    W = np.zeros((m, n), dtype=np.float64)
    for i in range(m):
        c = (f(i) + f(0.5)) * scale
        lo = max(0, int(c - sup + f(0.5)))
        hi = min(n, int(c + sup + f(0.5)))
        k = np.arange(lo, hi)
        w = _filter(code, ((k.astype(dtype) - c + f(0.5)) / fs).astype(dtype)).astype(dtype)
        s = dtype(0.0)
        for v in w:                                       # ascending, in `dtype`
            s = dtype(s + v)
        W[i, lo:hi] = (w / s).astype(dtype)
    return W


def _round_u8(x):
    return np.clip(np.floor(x + 0.5), 0, 255)


def resized_crop(img, box, out_hw, code, single_pass=False, dtype=np.float64):
    """uint8 [H, W, 3], box (top, left, height, width), (out_h, out_w) -> uint8 [out_h, out_w, 3]."""
    top, left, bh, bw = (int(v) for v in box)
    out_h, out_w = out_hw
    x = np.asarray(img)[top:top + bh, left:left + bw].astype(np.float64)
    Wx, Wy = axis_matrix(bw, out_w, code, dtype), axis_matrix(bh, out_h, code, dtype)
    hor = np.einsum("xk,hkc->hxc", Wx, x)
    if not single_pass:
        hor = _round_u8(hor)
    return _round_u8(np.einsum("yh,hxc->yxc", Wy, hor)).astype(np.uint8)


def pil_resized_crop(img, box, out_hw, code):
    from PIL import Image
    top, left, bh, bw = (int(v) for v in box)
    im = Image.fromarray(np.asarray(img, dtype=np.uint8)).crop((left, top, left + bw, top + bh))
    return np.asarray(im.resize((out_hw[1], out_hw[0]), code), dtype=np.uint8)


def compare(a, b):
    """-> (largest difference in levels, share of values that differ)."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int(d.max()), float((d != 0).mean())


def get_params(H, W, u, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision's RandomResizedCrop.get_params for an H x W image with the uniforms u [10, 4] in place of its draws
    -> (top, left, h, w), and the index of the accepted attempt (None: the fallback)."""
    area = H * W
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for t in range(10):
        target = area * (scale[0] + float(u[t][0]) * (scale[1] - scale[0]))
        ar = math.exp(log_ratio[0] + float(u[t][1]) * (log_ratio[1] - log_ratio[0]))
        w = int(round(math.sqrt(target * ar)))
        h = int(round(math.sqrt(target / ar)))
        if 0 < w <= W and 0 < h <= H:
            top = int(math.floor(float(u[t][2]) * (H - h + 1)))
            left = int(math.floor(float(u[t][3]) * (W - w + 1)))
            return (top, left, h, w), t
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return ((H - h) // 2, (W - w) // 2, h, w), None


def make_image(h, w, seed, kind="smooth"):
    """uint8 [h, w, 3]: "smooth" = low-frequency colour plus mild noise (what a photograph's statistics ask of a resampler),
    "noise" = independent uniform levels, "checker" = a 0 / 255 checkerboard of 2 x 2 cells."""
    rng = np.random.RandomState(seed)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy // 2 + xx // 2) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "noise":
        return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 3))
    for c in range(3):
        fy, fx, p = rng.uniform(0.02, 0.25), rng.uniform(0.02, 0.25), rng.uniform(0, 6.28)
        out[:, :, c] = 127.5 + 90.0 * np.sin(fy * yy + fx * xx + p) + rng.normal(0, 12.0, size=(h, w))
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


def kernel_cases():
    """The inputs of the kernel tests, shared by the host build (tests/test_input_cpu.py) and the GPU (tests/test_gpu_input.py):
    [dict(name, slot (h, w), out (h, w), filters, samples [(image uint8 [h, w, 3], box (top, left, height, width))])]."""
    S = make_image
    return [
        dict(name="down 23x17 -> 7x5", slot=(23, 17), out=(7, 5), filters=(2, 3), samples=[(S(23, 17, 1), (0, 0, 23, 17))]),
        dict(name="up 3x4 -> 16x16", slot=(12, 12), out=(16, 16), filters=(2, 3), samples=[(S(12, 12, 2), (4, 5, 3, 4))]),
        dict(name="box 1x1", slot=(8, 8), out=(4, 4), filters=(2, 3), samples=[(S(8, 8, 3), (3, 2, 1, 1))]),
        dict(name="offset box, dims < slot", slot=(64, 64), out=(16, 12), filters=(2, 3), samples=[(S(40, 56, 4), (5, 9, 30, 41))]),
        dict(name="identity", slot=(20, 20), out=(16, 16), filters=(2, 3), samples=[(S(20, 20, 5, "noise"), (2, 3, 16, 16))]),
        dict(name="scale 8", slot=(56, 40), out=(7, 5), filters=(2, 3), samples=[(S(56, 40, 6), (0, 0, 56, 40))]),
        dict(name="three samples", slot=(64, 64), out=(23, 29), filters=(2, 3),
             samples=[(S(64, 64, 7), (0, 0, 64, 64)), (S(53, 47, 8), (3, 5, 47, 41)), (S(50, 61, 9), (11, 1, 37, 59))]),
        dict(name="bands 300x200 -> 224x224", slot=(400, 256), out=(224, 224), filters=(2, 3),
             samples=[(S(300, 200, 10), (0, 0, 300, 200))]),
        # two levels, cells of 2 x 2, enlarged: the horizontal pass overshoots 0 / 255 and is clamped before the vertical one
        dict(name="checkerboard", slot=(23, 19), out=(50, 44), filters=(3,), samples=[(S(23, 19, 0, "checker"), (0, 0, 23, 19))]),
    ]


def stage(case, fill=0, outside_box=None):
    """-> src uint8 [B, slot_h, slot_w, 3] (every byte outside the images = `fill`; with `outside_box` given, every byte outside
    the crop BOXES is that value instead, inside the images too), dims int32 [B, 2], boxes int32 [B, 4]."""
    (sh, sw), B = case["slot"], len(case["samples"])
    src = np.full((B, sh, sw, 3), fill, dtype=np.uint8)
    dims, boxes = np.zeros((B, 2), np.int32), np.zeros((B, 4), np.int32)
    for b, (img, box) in enumerate(case["samples"]):
        h, w = img.shape[:2]
        dims[b], boxes[b] = (h, w), box
        if outside_box is None:
            src[b, :h, :w] = img
        else:
            t, l, bh, bw = box
            src[b] = outside_box
            src[b, t:t + bh, l:l + bw] = img[t:t + bh, l:l + bw]
    return src, dims, boxes


FILE_SIZES = ((60, 90), (90, 60), (128, 128), (200, 300), (333, 250), (480, 640), (500, 375), (700, 500))     # (h, w)


def make_files(root, n=48, seed=0):
    """n image files under `root`, sizes cycling through FILE_SIZES (60x90 ... 700x500), two JPEGs to one PNG
    -> [(path, caption)]; the captions are distinct."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    items = []
    for i in range(n):
        h, w = FILE_SIZES[i % len(FILE_SIZES)]
        a = make_image(h, w, seed * 1000 + i)
        png = i % 3 == 2
        path = os.path.join(root, "img_%03d.%s" % (i, "png" if png else "jpg"))
        if png:
            Image.fromarray(a).save(path)
        else:
            Image.fromarray(a).save(path, quality=90)
        items.append((path, "a photo of object number %d on the left" % i))
    return items


def write_manifest(path, items, root):
    with open(path, "w", encoding="utf-8") as f:
        for p, cap in items:
            f.write("%s\t%s\n" % (os.path.relpath(p, root), cap))
