"""The training input path without a GPU: include/msclip_input.h as msclip_amd/input_hip.py binds it, msclip_resized_crop's argument
validation (host side, before any launch), the fp64 restatement (tests/augment_ref.py) against PIL, the kernel body built for the
host (tests/input_host.cpp) against both, and the host logic: crop boxes, config settings, epoch order, the manifest, decoding."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import augment_ref as A
from conftest import ROOT
from msclip_amd import abi, augment, hip, input_hip, pairs
from msclip_amd._decode_worker import load_source
from msclip_amd.config import CfgNode, named_config

VP, CI = ctypes.c_void_p, ctypes.c_int
# the caps of the kernel tests (conditions, not measurements): (levels, share of values that differ)
CAP_REF, CAP_PIL = (1, 0.03), (2, 0.03)


# ---------------------------------------------------------------------------- the header and its binding
def test_input_header_binding():
    inp = abi.load(input_hip.HEADER, input_hip.VERSION_MACRO)
    assert os.path.basename(input_hip.HEADER) == "msclip_input.h" and inp.version == 1 == input_hip.INPUT_ABI_VERSION
    assert not inp.structs
    assert inp.protos == {
        "msclip_resized_crop_band": (CI, [CI, CI, CI, CI, CI]),
        "msclip_resized_crop_lds": (CI, [CI, CI, CI, CI, CI]),
        "msclip_resized_crop": (CI, [VP, CI, CI, VP, VP, VP, VP, CI, CI, CI, CI, VP, CI, VP, VP]),
        "msclip_input_abi_version": (CI, []),
    }
    assert input_hip.INPUT_EXPORTS == tuple(inp.protos)
    main = abi.load()
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    ext4 = abi.load(abi.EXT4_HEADER, abi.EXT4_VERSION_MACRO, known=tuple(main.structs) + tuple(ext3.structs))
    ext5 = abi.load(abi.EXT5_HEADER, abi.EXT5_VERSION_MACRO)
    for older in (main, ext, ext2, ext3, ext4, ext5):
        assert not set(inp.protos) & set(older.protos)
    assert [row[0] for row in hip._BOUND] == ["_ABI", "_EXT", "_EXT2", "_EXT3", "_EXT4", "_EXT5"]
    assert input_hip.CROP_MAX_SCALE == 8 and input_hip.CROP_LDS_BYTES == 65536
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = input_hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in input_hip.INPUT_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_input_abi_version() == 1


def test_plan_fits_the_lds_budget():
    """The band / LDS rule of the header, restated: the flagship shape, a shape whose band does not divide out_h, the limits."""
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    assert input_hip.crop_band(512, 512, 224, 224, 3) == 16 and input_hip.crop_lds(512, 512, 224, 224, 3) == 52800
    assert input_hip.crop_band(400, 256, 224, 224, 3) == 24                   # 224 = 9 * 24 + 8: a ragged last band
    for sh, sw, oh, ow in ((23, 17, 7, 5), (56, 40, 7, 5), (512, 512, 64, 64), (1792, 1792, 224, 224), (8, 8, 1, 1), (400, 256, 224, 224)):
        for f in (2, 3):
            band, lds = input_hip.crop_band(sh, sw, oh, ow, f), input_hip.crop_lds(sh, sw, oh, ow, f)
            assert 1 <= band <= min(32, oh) and 0 < lds <= input_hip.CROP_LDS_BYTES, (sh, sw, oh, ow, f, band, lds)
            S, sy, sx = f - 1, max(sh / oh, 1.0), max(sw / ow, 1.0)
            kx, ky = 2 * int(np.ceil(S * sx)) + 1, 2 * int(np.ceil(S * sy)) + 1
            rows = int(np.floor((band - 1) * sh / oh + 2 * S * sy)) + 2
            assert lds == 4 * ow * (kx + 2) + 4 * band * (ky + 2) + 4 * rows * ow
    assert input_hip.crop_band(57, 40, 7, 5, 3) == -1 and input_hip.crop_band(56, 41, 7, 5, 3) == -1       # beyond 8 x
    assert input_hip.crop_band(4096, 4096, 1024, 1024, 3) == -1                                           # one row does not fit


def test_resized_crop_rejections():
    """Every MSCLIP_EINVAL rule on fake non-null pointers: a call that got past its checks would launch on them."""
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = input_hip.lib()
    p, odd, two = VP(0x10000), VP(0x10001), VP(0x10002)

    def crop(src=p, sh=64, sw=64, dims=p, boxes=p, flip=p, lut=p, B=4, f=3, oh=16, ow=16, out=p, bf16=0, u8=p):
        return L.msclip_resized_crop(src, sh, sw, dims, boxes, flip, lut, B, f, oh, ow, out, bf16, u8, None)
    for name in ("src", "dims", "boxes", "lut", "out"):
        assert crop(**{name: None}) == -1, name                              # null
    for name in ("dims", "boxes", "flip", "lut", "out"):
        assert crop(**{name: two}) == -1, name                               # misaligned
    assert crop(out=odd, bf16=1) == -1                                       # bf16 output: 2 bytes
    assert crop(B=0) == -1 and crop(B=-3) == -1
    assert crop(oh=0) == -1 and crop(ow=0) == -1 and crop(oh=-1) == -1 and crop(ow=-16) == -1
    assert crop(sh=0) == -1 and crop(sw=-1) == -1
    for f in (0, 1, 4, 5, -2):
        assert crop(f=f) == -1, f
    assert crop(sh=129) == -1 and crop(sw=129) == -1                         # a slot beyond MSCLIP_CROP_MAX_SCALE x the output
    assert crop(sh=4096, sw=4096, oh=1024, ow=1024) == -1                    # a band of one row over the LDS budget
    assert crop(oh=64, ow=64, B=2 ** 31 - 1) == -1                           # two bands per sample: the grid passes 2^31 - 1


# ---------------------------------------------------------------------------- the restatement, PIL and the host build
def _per_case(fn):
    """(case name, filter) -> (largest difference, share of differing values) over all samples of the case."""
    out = {}
    for case in A.kernel_cases():
        for code in case["filters"]:
            a, b = zip(*(fn(case, code, i, img, box) for i, (img, box) in enumerate(case["samples"])))
            out[case["name"], code] = A.compare(np.concatenate([x.reshape(-1) for x in a]), np.concatenate([x.reshape(-1) for x in b]))
    return out


def test_restatement_against_pil():
    got = _per_case(lambda case, code, i, img, box: (A.resized_crop(img, box, case["out"], code),
                                                     A.pil_resized_crop(img, box, case["out"], code)))
    for key, (levels, share) in got.items():
        print(f"fp64 restatement vs PIL, {key}: {levels} levels, {100 * share:.2f} % differ")
        assert levels <= 2 and share <= 0.03, key
    # the uint8 intermediate is part of the definition: without it the two-level case is far off
    case = [c for c in A.kernel_cases() if c["name"] == "checkerboard"][0]
    img, box = case["samples"][0]
    single = A.resized_crop(img, box, case["out"], 3, single_pass=True)
    levels, share = A.compare(single, A.pil_resized_crop(img, box, case["out"], 3))
    print(f"single pass vs PIL on the checkerboard, bicubic: {levels} levels, {100 * share:.2f} % differ")
    assert levels > 10


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/input_host.cpp (the kernel body, msclip_amd/csrc/input_body.h) built with input.hip's floating-point flags."""
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, g++, or the clang++ that hipcc drives)"
    so = str(tmp_path_factory.mktemp("input_host") / "libinput_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "input_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def test_host_program_under_sanitizers(tmp_path):
    """tests/input_host.cpp as a stand-alone program under AddressSanitizer and UBSan: ragged shapes, boxes and sizes of INT_MIN /
    INT_MAX, an intermediate buffer of exactly the device's LDS size, and the plan's guards as assertions (CROP_GUARD)."""
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, g++, or the clang++ that hipcc drives)"
    exe = str(tmp_path / "input_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DINPUT_HOST_MAIN",
                    os.path.join(ROOT, "tests", "input_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "input_host: checksum" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _host_crop(L, case, code, flip=None, bf16=False, **stage):
    src, dims, boxes = A.stage(case, **stage)
    (oh, ow), B = case["out"], len(dims)
    lut = np.ascontiguousarray(np.random.RandomState(0).randn(3, 256).astype(np.float32))
    out = np.zeros((B, 3, oh, ow), np.uint16 if bf16 else np.float32)
    u8 = np.zeros((B, oh, ow, 3), np.uint8)
    P = lambda a: None if a is None else a.ctypes.data_as(VP)         # noqa: E731
    fl = None if flip is None else np.asarray(flip, np.int32)
    rc = L.host_resized_crop(P(src), src.shape[1], src.shape[2], P(dims), P(boxes), P(fl), P(lut), B, code, oh, ow, P(out), int(bf16),
                             P(u8))
    assert rc == 0
    return out, u8, lut


def test_host_build_of_the_kernel_body(host_lib):
    """The kernel's arithmetic on the CPU: on the inputs of the GPU test it stays under HALF of that test's caps (otherwise the
    inputs change, not the caps); outside pixels, flip, table and layout hold bitwise."""
    worst = {"ref": (0, 0.0), "pil": (0, 0.0)}
    for case in A.kernel_cases():
        assert host_lib.host_resized_crop_band(*case["slot"], *case["out"], 3) == input_hip.crop_band(*case["slot"], *case["out"], 3)
        for code in case["filters"]:
            out, u8, lut = _host_crop(host_lib, case, code, fill=7)
            ref = np.stack([A.resized_crop(img, box, case["out"], code) for img, box in case["samples"]])
            pil = np.stack([A.pil_resized_crop(img, box, case["out"], code) for img, box in case["samples"]])
            for what, other, cap in (("ref", ref, CAP_REF), ("pil", pil, CAP_PIL)):
                levels, share = A.compare(u8, other)
                print(f"host build vs {what}, {case['name']}, filter {code}: {levels} levels, {100 * share:.3f} % differ")
                assert levels <= cap[0] and share <= cap[1] / 2, (case["name"], code, what)
                worst[what] = (max(worst[what][0], levels), max(worst[what][1], share))
            assert np.array_equal(out, np.stack([lut[c][u8[..., c]] for c in range(3)], axis=1))
            out2, u82, _ = _host_crop(host_lib, case, code, fill=201, outside_box=93)
            assert np.array_equal(u8, u82) and np.array_equal(out, out2)
            B = len(case["samples"])
            outf, u8f, _ = _host_crop(host_lib, case, code, flip=[1] * B, fill=7)
            assert np.array_equal(u8f, u8[:, :, ::-1]) and np.array_equal(outf, out[..., ::-1])
            outb, _, _ = _host_crop(host_lib, case, code, bf16=True, fill=7)
            assert np.array_equal(outb, torch.from_numpy(out).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    print(f"host build, worst case: vs the restatement {worst['ref'][0]} levels / {100 * worst['ref'][1]:.2f} %, "
          f"vs PIL {worst['pil'][0]} levels / {100 * worst['pil'][1]:.2f} %")


# ---------------------------------------------------------------------------- crop boxes
def test_boxes_against_the_loop():
    g = torch.Generator().manual_seed(5)
    B = 2000
    sizes = torch.stack([torch.randint(1, 900, (B,), generator=g), torch.randint(1, 900, (B,), generator=g)], dim=1)
    forced = torch.tensor([[10, 400], [400, 10], [1, 1], [1, 700], [700, 1], [3, 2]])
    sizes[:60] = forced.repeat(10, 1)
    u = torch.rand(B, 10, 4, dtype=torch.float64, generator=g)
    for scale, ratio in (((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 1.0), (0.5, 2.0))):
        boxes = augment.random_resized_crop_boxes(sizes, u, scale, ratio)
        assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (B, 4)
        fallbacks = 0
        for b in range(B):
            H, W = int(sizes[b, 0]), int(sizes[b, 1])
            want, attempt = A.get_params(H, W, u[b].tolist(), scale, ratio)
            top, left, h, w = (int(v) for v in boxes[b])
            assert (top, left, h, w) == want, (b, H, W)
            assert 0 <= top and 0 <= left and 1 <= h and 1 <= w and top + h <= H and left + w <= W, (b, H, W, want)
            if attempt is None:
                fallbacks += 1
            else:                                        # w, h are rounded: each within half a pixel of its real value
                lo, hi = (w - 0.5) * (h - 0.5) / (H * W), (w + 0.5) * (h + 0.5) / (H * W)
                assert hi >= scale[0] - 1e-12 and lo <= scale[1] + 1e-12, (b, H, W, want)
        assert fallbacks >= 10                           # (the forced sizes)
    assert augment.random_resized_crop_boxes(sizes[:0], u[:0]).shape == (0, 4)
    with pytest.raises(ValueError):
        augment.random_resized_crop_boxes(sizes, u[:, :5])
    with pytest.raises(ValueError):
        augment.random_resized_crop_boxes(sizes.double(), u)


# ---------------------------------------------------------------------------- settings
def test_aug_settings_defaults_and_refusals():
    for name in ("b32-yfcc-msclips", "b32-laion-msclips", "b16-yfcc-msclips"):
        s = augment.aug_settings(named_config(name))
        assert s == dict(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), size=224, interpolation=3, mean=(0.485, 0.456, 0.406),
                         std=(0.229, 0.224, 0.225), flip_prob=0.0)
    s = augment.aug_settings(named_config("b32-yfcc-msclips", ["AUG.SCALE", "[0.3, 0.9]", "AUG.RATIO", "[0.5, 2.0]", "AUG.FLIP_PROB", "0.5",
                                                              "AUG.INTERPOLATION", "2", "TRAIN.IMAGE_SIZE", "[192, 192]"]))
    assert s["scale"] == (0.3, 0.9) and s["ratio"] == (0.5, 2.0) and s["flip_prob"] == 0.5 and s["interpolation"] == 2 and s["size"] == 192
    # the reference's own defaults are all off (lib/config/default.py:88-107): accepted
    off = CfgNode({"AUG": {"RANDOM_CENTER_CROP": False, "COLOR_JITTER": [0.4, 0.4, 0.4, 0.1, 0.0], "GRAY_SCALE": 0.0, "GAUSSIAN_BLUR": 0.0,
                           "MIXUP": 0.0, "MIXCUT": 0.0, "MIXCUT_MINMAX": [], "TIMM_AUG": {"USE_LOADER": False, "USE_TRANSFORM": False}}})
    assert augment.aug_settings(off)["scale"] == (0.08, 1.0)
    for key, value in (("AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 0.8]"), ("AUG.GRAY_SCALE", "0.2"), ("AUG.GAUSSIAN_BLUR", "0.5"),
                       ("AUG.MIXUP", "0.8"), ("AUG.MIXCUT", "1.0"), ("AUG.MIXCUT_MINMAX", "[0.2, 0.8]"), ("AUG.RANDOM_CENTER_CROP", "True"),
                       ("AUG.TIMM_AUG.USE_LOADER", "True"), ("AUG.TIMM_AUG.USE_TRANSFORM", "True")):
        with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
            augment.aug_settings(named_config("b32-yfcc-msclips", [key, value]))
    for key, value in (("AUG.INTERPOLATION", "1"), ("AUG.FLIP_PROB", "1.5"), ("AUG.SCALE", "[0.0, 1.0]"), ("TRAIN.IMAGE_SIZE", "[224, 192]")):
        with pytest.raises(ValueError):
            augment.aug_settings(named_config("b32-yfcc-msclips", [key, value]))


# ---------------------------------------------------------------------------- the epoch's order
def test_epoch_order():
    n, bs, world = 103, 4, 3
    ranks = [augment.epoch_order(n, 2, 7, r, world, bs) for r in range(world)]
    assert all(o.shape == (103 // 12, bs) and o.dtype == torch.int64 for o in ranks)      # whole batches, the same count on every rank
    flat = torch.cat([o.reshape(-1) for o in ranks])
    assert len(set(flat.tolist())) == flat.numel() == 96 and 0 <= int(flat.min()) and int(flat.max()) < n      # disjoint
    again = augment.epoch_order(n, 2, 7, 1, world, bs)
    assert torch.equal(again, ranks[1])
    assert not torch.equal(augment.epoch_order(n, 3, 7, 1, world, bs), ranks[1])          # another epoch
    assert not torch.equal(augment.epoch_order(n, 2, 8, 1, world, bs), ranks[1])          # another seed
    one = augment.epoch_order(n, 2, 7, 0, 1, bs)
    assert torch.equal(one.reshape(-1)[:96].reshape(-1, world)[:, 1], ranks[1].reshape(-1))      # rank r takes r::world
    assert augment.epoch_order(3, 0, 0, 0, 1, 4).shape == (0, 4)
    with pytest.raises(ValueError):
        augment.epoch_order(10, 0, 0, 2, 2, 4)


# ---------------------------------------------------------------------------- the manifest and decoding
def test_read_pairs(tmp_path):
    m = tmp_path / "pairs.tsv"
    m.write_text("a/x.jpg\ta photo of a café\n\nb.png\tleft\tof the tab\r\n", encoding="utf-8")
    assert pairs.read_pairs(str(m), "/data") == [("/data/a/x.jpg", "a photo of a café"), ("/data/b.png", "left\tof the tab")]
    m.write_text("no tab here\n", encoding="utf-8")
    with pytest.raises(ValueError, match="pairs.tsv:1"):
        pairs.read_pairs(str(m))


def test_load_source(tmp_path):
    from PIL import Image
    a = A.make_image(700, 500, 1)
    Image.fromarray(a).save(tmp_path / "big.jpg", quality=92)
    Image.fromarray(a).save(tmp_path / "big.png")
    Image.fromarray(a[:90, :60]).save(tmp_path / "small.jpg", quality=92)
    big = load_source(str(tmp_path / "big.jpg"), 128)                        # both sides > 2 * 128: draft takes 1/2, reduce(3) the rest
    assert big.dtype == np.uint8 and big.shape[2] == 3 and max(big.shape[:2]) <= 128 and big.shape[:2] == (117, 84)
    with Image.open(tmp_path / "big.jpg") as im:
        im.draft("RGB", (128, 128))
        assert im.size == (250, 350)                                         # the decoder did the coarse step: no 700 x 500 decode
        assert np.array_equal(big, np.asarray(im.convert("RGB").reduce(3)))
    png = load_source(str(tmp_path / "big.png"), 128)                        # no draft mode: reduce(6)
    assert png.shape == (117, 84, 3) and np.array_equal(png, np.asarray(Image.fromarray(a).reduce(6)))
    assert load_source(str(tmp_path / "big.png"), 512).shape == (350, 250, 3)
    assert np.array_equal(load_source(str(tmp_path / "big.png"), 700), a)    # fits: untouched
    small = load_source(str(tmp_path / "small.jpg"), 128)
    assert small.shape == (90, 60, 3)
    rgba = np.dstack([a[:40, :30], np.full((40, 30), 128, np.uint8)])
    Image.fromarray(rgba, "RGBA").save(tmp_path / "rgba.png")
    Image.fromarray(a[:40, :30]).convert("P").save(tmp_path / "pal.png")
    Image.fromarray(a[:40, :30, 0]).save(tmp_path / "grey.png")
    for name in ("rgba.png", "pal.png", "grey.png"):
        x = load_source(str(tmp_path / name), 64)
        assert x.shape == (40, 30, 3) and x.dtype == np.uint8, name
    assert np.array_equal(load_source(str(tmp_path / "rgba.png"), 64), a[:40, :30])
    files = A.make_files(str(tmp_path / "set"), n=9)
    assert [load_source(p, 512).shape[:2] for p, _ in files[:8]] == [(60, 90), (90, 60), (128, 128), (200, 300), (333, 250),
                                                                       (240, 320), (500, 375), (350, 250)]
