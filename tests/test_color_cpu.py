"""The colour stage of the training input path without a GPU: include/msclip_color.h as msclip_amd/color_hip.py binds it,
msclip_color_augment's argument validation (host side, before any launch), the numpy restatement (tests/color_ref.py) against PIL
and scipy, the kernel body built for the host (tests/color_host.cpp) against the restatement, and the host logic: colour_params,
blur_weights and aug_settings(colour=True)."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import color_ref as C
from conftest import ROOT
from msclip_amd import abi, augment, color_hip, hip, input_hip
from msclip_amd.config import named_config

VP, CI = ctypes.c_void_p, ctypes.c_int
FACTORS = (0.0, 0.6, 0.83, 1.0, 1.17, 1.4, 2.0)
SHIFTS = tuple(int(f * 255) & 255 for f in (0.5, -0.5, 0.1, -0.1, 0.05, 0.0))
BLUR_SHAPES = ((1, 4), (3, 9), (7, 5), (16, 16), (33, 20), (224, 224))
IMAGES = {"random": C.make_image(37, 29, 1), "low contrast": C.make_image(37, 29, 2, "low"), "r = g = b": C.make_image(37, 29, 3, "gray")}


def _build():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()


# ---------------------------------------------------------------------------- the header and its binding
def test_color_header_binding():
    col = abi.load(color_hip.HEADER, color_hip.VERSION_MACRO)
    assert os.path.basename(color_hip.HEADER) == "msclip_color.h" and col.version == 1 == color_hip.COLOR_ABI_VERSION
    assert not col.structs
    assert col.protos == {
        "msclip_color_augment_band": (CI, [CI, CI]),
        "msclip_color_augment_lds": (CI, [CI, CI]),
        "msclip_color_augment": (CI, [VP, VP, VP, VP, CI, CI, CI, CI, VP, VP, CI, VP, VP]),
        "msclip_color_abi_version": (CI, []),
    }
    assert color_hip.COLOR_EXPORTS == tuple(col.protos)
    main = abi.load()
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    ext4 = abi.load(abi.EXT4_HEADER, abi.EXT4_VERSION_MACRO, known=tuple(main.structs) + tuple(ext3.structs))
    ext5 = abi.load(abi.EXT5_HEADER, abi.EXT5_VERSION_MACRO)
    inp = abi.load(input_hip.HEADER, input_hip.VERSION_MACRO)
    for older in (main, ext, ext2, ext3, ext4, ext5, inp):
        assert not set(col.protos) & set(older.protos)
    assert [row[0] for row in hip._BOUND] == ["_ABI", "_EXT", "_EXT2", "_EXT3", "_EXT4", "_EXT5"]
    assert color_hip.COLOR_RADIUS == 6 == augment.BLUR_RADIUS and color_hip.COLOR_LDS_BYTES == 65536
    _build()
    L = color_hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in color_hip.COLOR_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_color_abi_version() == 1


def test_plan_fits_the_lds_budget():
    """The band / LDS rule of the header, restated."""
    _build()
    assert color_hip.augment_band(224, 224) == 24 and color_hip.augment_lds(224, 224) == 64512
    for H, W in ((7, 5), (16, 16), (33, 20), (64, 64), (224, 224), (1, 1), (5, 630), (1000, 300), (384, 384)):
        band, lds = color_hip.augment_band(H, W), color_hip.augment_lds(H, W)
        fits = [c for c in (32, 24, 16, 12, 8, 6, 4, 3, 2, 1) if 8 * (min(c, H) + 12) * W <= 65536]
        assert band == min(fits[0], H) and lds == 8 * (band + 12) * W <= color_hip.COLOR_LDS_BYTES, (H, W, band, lds)
    assert color_hip.augment_band(5, 631) == -1 and color_hip.augment_lds(5, 631) == -1       # one row does not fit
    assert color_hip.augment_band(0, 5) == -1 and color_hip.augment_band(5, -1) == -1


def test_color_augment_rejections():
    """Every MSCLIP_EINVAL rule on fake non-null pointers: a call that got past its checks would launch on them."""
    _build()
    L = color_hip.lib()
    p, q, odd, two = VP(0x10000), VP(0x20000), VP(0x10001), VP(0x10002)

    def aug(src=p, ops=p, coef=p, lut=p, B=4, H=16, W=16, stages=7, work=p, out=p, bf16=0, u8=q):
        return L.msclip_color_augment(src, ops, coef, lut, B, H, W, stages, work, out, bf16, u8, None)
    for name in ("src", "ops", "coef", "lut", "out"):
        assert aug(**{name: None}) == -1, name                               # null
    for stages in (1, 3, 5, 7):
        assert aug(work=None, stages=stages) == -1                           # jitter needs its scratch
    for name in ("ops", "coef", "lut", "work", "out"):
        assert aug(**{name: two}) == -1, name                                # misaligned
    assert aug(work=two, stages=6) == -1
    assert aug(out=odd, bf16=1) == -1                                        # bf16 output: 2 bytes
    assert aug(B=0) == -1 and aug(B=-3) == -1
    assert aug(H=0) == -1 and aug(W=0) == -1 and aug(H=-1) == -1 and aug(W=-16) == -1
    assert aug(stages=-1) == -1 and aug(stages=8) == -1
    assert aug(u8=p) == -1                                                   # in place: the blur reads neighbours
    assert aug(W=631) == -1 and aug(W=631, stages=0) == -1                   # a band of one row over the LDS budget
    assert aug(H=64, W=64, B=2 ** 31 - 1) == -1                              # two bands per image: the grid passes 2^31 - 1


# ---------------------------------------------------------------------------- the restatement against PIL and scipy
@pytest.mark.parametrize("name", list(IMAGES))
def test_restatement_ops_against_pil(name):
    img = IMAGES[name]
    assert np.array_equal(C.grayscale(img), C.pil_gray(img))
    for f in FACTORS:
        for op, fn in ((0, C.brightness), (1, C.contrast), (2, C.saturation)):
            assert np.array_equal(fn(img, f), C.pil_enhance(img, op, f)), (name, op, f)
    for q in SHIFTS:
        assert np.array_equal(C.hue(img, q), C.pil_hue(img, q)), (name, q)


def test_restatement_hsv_lattice_against_pil():
    from PIL import Image
    v = np.arange(0, 256, 5, dtype=np.uint8)
    lattice = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 52, 3)
    rand = C.make_image(200, 200, 9)
    for img in (lattice, rand):
        hsv = np.asarray(Image.fromarray(img).convert("HSV"), dtype=np.uint8)
        assert np.array_equal(C.rgb_to_hsv(img), hsv)
        assert np.array_equal(C.hsv_to_rgb(img), np.asarray(Image.fromarray(img, "HSV").convert("RGB"), dtype=np.uint8))


@pytest.mark.parametrize("name", list(IMAGES))
def test_restatement_orders_against_pil(name):
    """All 24 orders chained, then gray."""
    img = IMAGES[name]
    factors = (0.83, 1.4, 0.6)
    for order in itertools.permutations(range(4)):
        ours = C.grayscale(C.jitter(img, order, factors, 26))
        assert np.array_equal(ours, C.pil_gray(C.pil_jitter(img, order, factors, 26))), (name, order)
        assert np.array_equal(C.jitter(img, order, factors, 231), C.pil_jitter(img, order, factors, 231)), (name, order)


@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=["%dx%d" % s for s in BLUR_SHAPES])
def test_restatement_blur_against_scipy(shape):
    """At most 1 level on at most 0.1 % of the values: a cap, not a measurement."""
    for kind in ("noise", "smooth"):
        img = C.make_image(shape[0], shape[1], 5, kind)
        for sigma in (0.1, 0.7, 2.0):
            ours, ref = C.blur(img, C.weights(sigma)), C.scipy_blur(img, sigma)
            d = np.abs(ours.astype(np.int32) - ref.astype(np.int32))
            print(f"blur {shape} {kind} sigma {sigma}: {int(d.max())} levels, {100 * float((d != 0).mean()):.4f} % differ")
            assert d.max() <= 1 and (d != 0).mean() <= 1e-3, (shape, kind, sigma)
            if sigma == 0.1:
                assert np.array_equal(ours, img)                                 # the identity


def test_mirror():
    for n in (1, 2, 3, 5, 7):
        for j in range(-20, 25):
            want = np.pad(np.arange(n), 30, mode="reflect")[j + 30] if n > 1 else 0
            assert int(C.mirror(j, n)) == want, (j, n)


# ---------------------------------------------------------------------------- the kernel body on the host
def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, g++, or the clang++ that hipcc drives)"
    return cxx


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/color_host.cpp (the kernel body, msclip_amd/csrc/color_body.h) built with color.hip's floating-point flags."""
    so = str(tmp_path_factory.mktemp("color_host") / "libcolor_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "color_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def test_host_program_under_sanitizers(tmp_path):
    """tests/color_host.cpp as a stand-alone program under AddressSanitizer and UBSan: ragged shapes, every `stages` mask, ops of
    INT_MIN / INT_MAX, NaN / Inf factors and weights, and LDS buffers of exactly the device's size."""
    exe = str(tmp_path / "color_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DCOLOR_HOST_MAIN",
                    os.path.join(ROOT, "tests", "color_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "color_host: checksum" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _host(L, src, ops, coef, lut, stages=7, bf16=False):
    B, H, W = src.shape[:3]
    out = np.zeros((B, 3, H, W), np.uint16 if bf16 else np.float32)
    u8 = np.zeros((B, H, W, 3), np.uint8)
    work = np.zeros(B, np.int32)
    P = lambda a: a.ctypes.data_as(VP)                                # noqa: E731
    src, ops, coef = np.ascontiguousarray(src), np.ascontiguousarray(ops), np.ascontiguousarray(coef)
    assert L.host_color_augment(P(src), P(ops), P(coef), P(lut), B, H, W, stages, P(work), P(out), int(bf16), P(u8)) == 0
    return out, u8


@pytest.mark.parametrize("shape", ((7, 5), (16, 16), (33, 20), (64, 64), (1, 4), (70, 41)), ids=lambda s: "%dx%d" % s)
def test_host_build_of_the_kernel_body(host_lib, shape):
    """Bitwise the restatement: out_u8 and out, fp32 and bf16, every `stages` mask."""
    _build()
    assert host_lib.host_color_augment_band(*shape) == color_hip.augment_band(*shape)
    src, ops, coef = C.batch6(*shape)
    lut = np.ascontiguousarray(np.random.RandomState(0).randn(3, 256).astype(np.float32))
    for stages in (7, 0, 1, 2, 4, 3):
        want = C.augment_u8(src, ops, coef, stages)
        out, u8 = _host(host_lib, src, ops, coef, lut, stages)
        assert np.array_equal(u8, want), (shape, stages, np.argwhere(u8 != want)[:5])
        assert np.array_equal(out, C.lookup(want, lut))
    outb, u8b = _host(host_lib, src, ops, coef, lut, 7, bf16=True)
    assert np.array_equal(u8b, want_all := C.augment_u8(src, ops, coef, 7))
    assert np.array_equal(outb, torch.from_numpy(C.lookup(want_all, lut)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    # a weight that is not a number counts as 0; an accumulator that is not a number gives 0
    coef[0, 5], coef[2, 4:11] = float("nan"), [3e38, -3e38, 3e38, 1, 1, 1, 1]
    _, u8 = _host(host_lib, src, ops, coef, lut, 7)
    assert np.array_equal(u8, C.augment_u8(src, ops, coef, 7))


# ---------------------------------------------------------------------------- colour_params, blur_weights, settings
SET = dict(color_jitter=(0.4, 0.3, 0.2, 0.1, 0.8), gray_scale=0.2, gaussian_blur=0.5)


def test_blur_weights():
    sig = torch.tensor([0.1, 0.7, 2.0, 1.234])
    w = augment.blur_weights(sig)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4, 7)
    for i, s in enumerate(sig.double().tolist()):
        assert np.array_equal(w[i].numpy(), C.weights(s))
        assert abs(float(w[i, 0].double() + 2 * w[i, 1:].double().sum()) - 1.0) < 1e-6
    assert w[0, 0] == 1.0 and float(w[0, 1]) < 1e-20 and (w[0, 2:] == 0.0).all()           # sigma 0.1: the identity
    assert tuple(augment.blur_weights(0.5).shape) == (7,)


def test_colour_params_ranges_and_ends():
    g = torch.Generator().manual_seed(1)
    u = torch.rand(4000, 9, dtype=torch.float64, generator=g)
    ops, coef = augment.colour_params(u, SET)
    assert ops.dtype == torch.int32 and tuple(ops.shape) == (4000, 8) and coef.dtype == torch.float32 and tuple(coef.shape) == (4000, 12)
    jit = u[:, 0] < 0.8
    assert torch.equal((ops[:, :4] >= 0).all(dim=1), jit) and torch.equal((ops[:, :4] == -1).all(dim=1), ~jit)
    assert all(sorted(row) == [0, 1, 2, 3] for row in ops[jit][:, :4].tolist())
    assert len({tuple(row) for row in ops[jit][:, :4].tolist()}) == 24                   # every order is reachable
    for col, x in enumerate((0.4, 0.3, 0.2)):
        f = coef[jit][:, col].double()
        assert f.min() >= 1 - x - 1e-6 and f.max() <= 1 + x + 1e-6 and f.max() - f.min() > 1.9 * x
        assert (coef[~jit][:, col] == 1.0).all()
    shift = ops[:, 4].long()
    assert ((shift >= 0) & (shift <= 255)).all() and (shift[~jit] == 0).all()
    signed = torch.where(shift > 127, shift - 256, shift)
    assert signed.min() == -25 and signed.max() == 25                                    # int(+-0.1 * 255), truncated toward zero
    assert torch.equal(ops[:, 5] != 0, u[:, 6] < 0.2) and torch.equal(ops[:, 6] != 0, u[:, 7] < 0.5) and (ops[:, 7] == 0).all()
    assert (coef[:, 3] == 0).all() and (coef[:, 11] == 0).all()
    blur = ops[:, 6] != 0
    assert torch.equal(coef[blur][:, 4:11], augment.blur_weights(0.1 + 1.9 * u[blur][:, 8]))
    skip = torch.tensor([1.0, 0, 0, 0, 0, 0, 0])
    assert (coef[~blur][:, 4:11] == skip).all()
    # both ends of every uniform
    eps = 1.0 - 2.0 ** -53
    lo, hi = augment.colour_params(torch.zeros(1, 9, dtype=torch.float64), SET), augment.colour_params(torch.full((1, 9), eps, dtype=torch.float64), SET)
    assert lo[0][0].tolist() == [0, 1, 2, 3, (-25) & 255, 1, 1, 0] and hi[0][0].tolist() == [-1, -1, -1, -1, 0, 0, 0, 0]
    assert np.allclose(lo[1][0, :3].numpy(), [0.6, 0.7, 0.8]) and np.array_equal(lo[1][0, 4:11].numpy(), C.weights(0.1))
    always = dict(color_jitter=(0.4, 2.0, 0.2, 0.5, 1.0), gray_scale=1.0, gaussian_blur=1.0)
    o, c = augment.colour_params(torch.full((1, 9), eps, dtype=torch.float64), always)
    assert o[0].tolist() == [3, 2, 1, 0, 127, 1, 1, 0] and np.allclose(c[0, :3].numpy(), [1.4, 3.0, 1.2])
    assert np.array_equal(c[0, 4:11].numpy(), C.weights(0.1 + 1.9 * eps))
    o, c = augment.colour_params(torch.zeros(1, 9, dtype=torch.float64), always)
    assert o[0].tolist() == [0, 1, 2, 3, (-127) & 255, 1, 1, 0] and np.allclose(c[0, :3].numpy(), [0.6, 0.0, 0.8])      # max(0, 1 - 2)


def test_colour_params_skips():
    u = torch.rand(500, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    skip_ops, skip_coef = [-1, -1, -1, -1, 0, 0, 0, 0], [1.0, 1.0, 1.0, 0.0, 1.0] + [0.0] * 7
    for settings in (dict(color_jitter=(0.4, 0.4, 0.4, 0.1, 0.0), gray_scale=0.0, gaussian_blur=0.0), {}):      # p = 0: all-skip records
        ops, coef = augment.colour_params(u, settings)
        assert (ops == torch.tensor(skip_ops, dtype=torch.int32)).all() and (coef == torch.tensor(skip_coef)).all()
        assert augment.colour_stages(settings) == 0
    # zero strength drops the op
    ops, coef = augment.colour_params(u, dict(color_jitter=(0.4, 0.0, 0.4, 0.0, 1.0)))
    assert not ((ops[:, :4] == 1) | (ops[:, :4] == 3)).any() and (ops[:, 4] == 0).all() and (coef[:, 1] == 1.0).all()
    assert all(sorted(r) == [-1, -1, 0, 2] for r in ops[:, :4].tolist())
    assert augment.colour_stages(dict(color_jitter=(0.4, 0.0, 0.4, 0.0, 1.0))) == 1
    assert augment.colour_stages(dict(color_jitter=(0.0, 0.0, 0.0, 0.0, 1.0), gray_scale=0.1)) == 2
    assert augment.colour_stages(SET) == 7
    with pytest.raises(ValueError):
        augment.colour_params(u[:, :8], SET)
    # the order index: floor(24 u) into the lexicographic permutations
    perms = list(itertools.permutations(range(4)))
    uu = torch.zeros(24, 9, dtype=torch.float64)
    uu[:, 1] = (torch.arange(24, dtype=torch.float64) + 0.5) / 24
    ops, _ = augment.colour_params(uu, dict(color_jitter=(0.1, 0.1, 0.1, 0.1, 1.0)))
    assert [tuple(r) for r in ops[:, :4].tolist()] == perms == C.ORDERS


def test_aug_settings_colour():
    base = dict(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), size=224, interpolation=3, mean=(0.485, 0.456, 0.406),
                std=(0.229, 0.224, 0.225), flip_prob=0.0)
    cfg = named_config("b32-yfcc-msclips")
    assert augment.aug_settings(cfg) == base                                 # the default call: unchanged
    s = augment.aug_settings(cfg, colour=True)
    assert {k: s[k] for k in base} == base and set(s) == set(base) | {"color_jitter", "gray_scale", "gaussian_blur"}
    assert s["color_jitter"][4] == 0.0 and s["gray_scale"] == 0.0 and s["gaussian_blur"] == 0.0 and augment.colour_stages(s) == 0
    # (the named configs leave every colour switch off)
    on = named_config("b32-yfcc-msclips", ["AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 0.8]", "AUG.GRAY_SCALE", "0.2", "AUG.GAUSSIAN_BLUR", "0.5"])
    with pytest.raises(NotImplementedError, match=r"AUG\.COLOR_JITTER"):
        augment.aug_settings(on)
    s = augment.aug_settings(on, colour=True)
    assert s == dict(base, color_jitter=(0.4, 0.4, 0.4, 0.1, 0.8), gray_scale=0.2, gaussian_blur=0.5) and augment.colour_stages(s) == 7
    for key, value in (("AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 1.5]"), ("AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, -0.1]"),
                       ("AUG.COLOR_JITTER", "[-0.4, 0.4, 0.4, 0.1, 0.8]"), ("AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.6, 0.8]"),
                       ("AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.8]"), ("AUG.GRAY_SCALE", "1.2"), ("AUG.GRAY_SCALE", "-0.2"),
                       ("AUG.GAUSSIAN_BLUR", "2.0"), ("AUG.GAUSSIAN_BLUR", "-1.0")):
        with pytest.raises(ValueError):
            augment.aug_settings(named_config("b32-yfcc-msclips", [key, value]), colour=True)
    for key, value in (("AUG.MIXUP", "0.8"), ("AUG.MIXCUT", "1.0"), ("AUG.MIXCUT_MINMAX", "[0.2, 0.8]"), ("AUG.RANDOM_CENTER_CROP", "True"),
                       ("AUG.TIMM_AUG.USE_LOADER", "True"), ("AUG.TIMM_AUG.USE_TRANSFORM", "True")):
        with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
            augment.aug_settings(named_config("b32-yfcc-msclips", [key, value]), colour=True)
