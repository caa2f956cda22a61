"""The training input path on the GPU: msclip_resized_crop (include/msclip_input.h) against the fp64 restatement of
tests/augment_ref.py and against PIL on the shared kernel cases, its bitwise properties (pixels outside the box, table and layout,
flip, repeatability), msclip_amd.pairs.PairPipeline on generated files (content, replay, resume) and tools/train_pairs.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref as A
from conftest import ROOT
from msclip_amd import augment, input_hip, pairs, zeroshot
from msclip_amd._decode_worker import load_source
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu

# conditions, not measurements (largest difference in levels, share of values that differ); the host build of the kernel body
# stays under half of each on these inputs (tests/test_input_cpu.py)
CAP_REF, CAP_PIL = (1, 0.03), (2, 0.03)
CASES = A.kernel_cases()
_REF = {}


def _reference(ci, code):
    """(restatement, PIL) uint8 [B, out_h, out_w, 3] of case ci, computed once."""
    if (ci, code) not in _REF:
        case = CASES[ci]
        _REF[ci, code] = (np.stack([A.resized_crop(img, box, case["out"], code) for img, box in case["samples"]]),
                          np.stack([A.pil_resized_crop(img, box, case["out"], code) for img, box in case["samples"]]))
    return _REF[ci, code]


def _lut(dev):
    return torch.from_numpy(np.random.RandomState(0).randn(3, 256).astype(np.float32)).to(dev)


def _run(dev, case, code, flip=None, bf16=False, **stage):
    src, dims, boxes = A.stage(case, **stage)
    fl = None if flip is None else torch.tensor(flip, dtype=torch.int32, device=dev)
    out, u8 = input_hip.resized_crop(torch.from_numpy(src).to(dev), torch.from_numpy(dims).to(dev), torch.from_numpy(boxes).to(dev),
                                     _lut(dev), case["out"], flip=fl, filter=code, bf16=bf16, want_u8=True)
    torch.cuda.synchronize()
    return out, u8


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_resized_crop_cases(gpu_device, ci):
    case = CASES[ci]
    B = len(case["samples"])
    for code in case["filters"]:
        out, u8 = _run(gpu_device, case, code, fill=7)
        ref, pil = _reference(ci, code)
        got = u8.cpu().numpy()
        for what, other, cap in (("the restatement", ref, CAP_REF), ("PIL", pil, CAP_PIL)):
            levels, share = A.compare(got, other)
            print(f"{case['name']}, filter {code}, vs {what}: {levels} levels, {100 * share:.3f} % of {got.size} values differ")
            assert levels <= cap[0] and share <= cap[1], (case["name"], code, what, levels, share)
        # table and layout: out is lut[ch][out_u8] in NCHW, bitwise; bf16 is the rounded fp32 value
        lut = _lut(gpu_device)
        want = torch.stack([lut[c][u8[..., c].long()] for c in range(3)], dim=1)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3) + tuple(case["out"]) and torch.equal(out, want)
        outb, u8b = _run(gpu_device, case, code, bf16=True, fill=7)
        assert outb.dtype == torch.bfloat16 and torch.equal(outb, out.to(torch.bfloat16)) and torch.equal(u8b, u8)
        # nothing outside the crop box is read: other bytes everywhere else, inside the image and in the slot's padding
        out2, u82 = _run(gpu_device, case, code, fill=201, outside_box=93)
        assert torch.equal(u82, u8) and torch.equal(out2, out)
        # flip: the same result with its columns reversed, sample by sample
        flip = [1] + [0] * (B - 1) if B > 1 else [1]
        outf, u8f = _run(gpu_device, case, code, flip=flip, fill=7)
        for b, f in enumerate(flip):
            assert torch.equal(u8f[b], u8[b].flip(1) if f else u8[b]) and torch.equal(outf[b], out[b].flip(2) if f else out[b])
        # repeatability
        out3, u83 = _run(gpu_device, case, code, fill=7)
        assert torch.equal(u83, u8) and torch.equal(out3, out)


def test_resized_crop_wrapper_refuses(gpu_device):
    dev = gpu_device
    src = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device=dev)
    dims, boxes = torch.zeros(2, 2, dtype=torch.int32, device=dev), torch.zeros(2, 4, dtype=torch.int32, device=dev)
    lut = _lut(dev)
    for bad in (dict(src=src.float()), dict(dims=dims.long()), dict(boxes=boxes[:1]), dict(lut=lut[:2]), dict(filter=1),
                dict(size=3), dict(size=(0, 4)), dict(src=src.cpu())):
        args = dict(src=src, dims=dims, boxes=boxes, lut=lut, size=16, filter=3)
        args.update(bad)
        with pytest.raises(ValueError):
            input_hip.resized_crop(args.pop("src"), args.pop("dims"), args.pop("boxes"), args.pop("lut"), args.pop("size"), **args)


def test_resized_crop_clamps_boxes_and_dims(gpu_device):
    """Sizes and boxes outside their ranges are clamped on the device, value by value (include/msclip_input.h): the launch gives
    the pixels of the clamped box -- bitwise what a launch with the clamped values gives, and within the kernel tests' cap of the
    restatement on that box."""
    dev = gpu_device
    imgs = [A.make_image(32, 32, 21, "noise"), A.make_image(32, 32, 22, "noise")]
    src = torch.from_numpy(np.stack(imgs)).to(dev)
    lut = _lut(dev)
    big, small = (1 << 31) - 1, -(1 << 31)
    wild_dims = torch.tensor([[32, 32], [-5, 1 << 30]], dtype=torch.int32, device=dev)
    wild_boxes = torch.tensor([[-9, 40, 1 << 30, -1], [small, big, big, 0]], dtype=torch.int32, device=dev)
    # (h, w) into [1, slot]; top into [0, h - 1], left into [0, w - 1], height into [1, h - top], width into [1, w - left]
    dims = torch.tensor([[32, 32], [1, 32]], dtype=torch.int32, device=dev)
    boxes = torch.tensor([[0, 31, 32, 1], [0, 31, 1, 1]], dtype=torch.int32, device=dev)
    for code in (2, 3):
        out, u8 = input_hip.resized_crop(src, wild_dims, wild_boxes, lut, 16, filter=code, want_u8=True)
        want, want_u8 = input_hip.resized_crop(src, dims, boxes, lut, 16, filter=code, want_u8=True)
        assert torch.equal(u8, want_u8) and torch.equal(out, want)
        for b in range(2):
            ref = A.resized_crop(imgs[b], boxes[b].tolist(), (16, 16), code)
            levels, share = A.compare(u8[b].cpu().numpy(), ref)
            assert levels <= CAP_REF[0] and share <= CAP_REF[1], (code, b, levels, share)
        assert torch.equal(u8[1], src[1, 0, 31].view(1, 1, 3).expand(16, 16, 3))          # a 1 x 1 box: that pixel everywhere


# ---------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pairs"))
    items = A.make_files(root, n=48)
    A.write_manifest(os.path.join(root, "pairs.tsv"), items, root)
    return root, items


@pytest.fixture(scope="module")
def tokenizer():
    from msclip_amd.tokenizer import SimpleTokenizer
    return SimpleTokenizer()


def _settings(**over):
    return dict(augment.aug_settings(named_config("b32-yfcc-msclips")), **over)


def test_pipeline_content(gpu_device, files, tokenizer):
    root, items = files
    assert pairs.read_pairs(os.path.join(root, "pairs.tsv"), root) == items
    settings = _settings(flip_prob=0.5)
    pipe = pairs.PairPipeline(items, 16, gpu_device, settings, tokenizer=tokenizer, seed=3, workers=8)
    lut = zeroshot.normalise_lut(settings["mean"], settings["std"]).to(gpu_device)
    seen, flips = [], 0
    for img, tok, index in pipe:
        assert img.dtype == torch.float32 and tuple(img.shape) == (16, 3, 224, 224) and img.device == gpu_device
        assert tok.dtype == torch.int64 and tuple(tok.shape) == (16, 77) and tok.device == gpu_device
        src = torch.zeros(16, 512, 512, 3, dtype=torch.uint8)
        for j, i in enumerate(index.tolist()):
            a = load_source(items[i][0], 512)
            src[j, :a.shape[0], :a.shape[1]] = torch.from_numpy(a)
            assert tuple(pipe.last_dims[j].tolist()) == a.shape[:2]
            t, l, h, w = pipe.last_boxes[j].tolist()
            assert 0 <= t and 0 <= l and h >= 1 and w >= 1 and t + h <= a.shape[0] and l + w <= a.shape[1]
        want = input_hip.resized_crop(src.to(gpu_device), pipe.last_dims.to(gpu_device), pipe.last_boxes.to(gpu_device), lut, 224,
                                      flip=pipe.last_flip.to(gpu_device), filter=settings["interpolation"])
        assert torch.equal(img, want)
        assert torch.equal(tok.cpu(), tokenizer([items[i][1] for i in index.tolist()]))
        seen += index.tolist()
        flips += int(pipe.last_flip.sum())
    assert sorted(seen) == list(range(48)) and 0 < flips < 48
    pipe.close()


def test_pipeline_replay_and_resume(gpu_device, files, tokenizer):
    _, items = files
    settings = _settings(size=64)

    def run(pipe, n=None):
        out = []
        for img, tok, index in pipe:
            out.append((img.clone(), tok.clone(), index.clone(), pipe.last_boxes.clone()))
            if n is not None and len(out) == n:
                break
        return out

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    p1 = pairs.PairPipeline(items, 8, gpu_device, settings, tokenizer=tokenizer, seed=11, workers=8, slot=256)
    first = run(p1)
    assert len(first) == 6 == len(p1)
    p2 = pairs.PairPipeline(items, 8, gpu_device, settings, tokenizer=tokenizer, seed=11, workers=3, slot=256)
    assert same(run(p2), first)                              # the same seed: the same batches, whatever the workers' timing
    p2.set_epoch(1)
    second = run(p2)
    assert len(second) == 6
    assert not torch.equal(torch.cat([b[2] for b in second]), torch.cat([b[2] for b in first]))            # another order
    assert not torch.equal(torch.cat([b[3] for b in second]), torch.cat([b[3] for b in first]))            # other boxes
    p2.set_epoch(0)
    assert same(run(p2), first)                              # an epoch depends on (seed, epoch) alone
    # resume: the state after batch 1, loaded into a fresh pipeline, continues with batches 2, 3, ...
    p3 = pairs.PairPipeline(items, 8, gpu_device, settings, tokenizer=tokenizer, seed=11, workers=8, slot=256)
    head = run(p3, 2)
    state = p3.state_dict()
    assert same(head, first[:2]) and state["epoch"] == 0 and state["pos"] == 2
    p4 = pairs.PairPipeline(items, 8, gpu_device, settings, tokenizer=tokenizer, seed=99, workers=8, slot=256)
    p4.load_state_dict(state)
    assert same(run(p4), first[2:])
    assert same(run(p3), first[2:])                          # and the interrupted one itself goes on where it stopped
    with pytest.raises(ValueError):
        pairs.PairPipeline(items, 4, gpu_device, settings, tokenizer=tokenizer, slot=256).load_state_dict(state)
    for p in (p1, p2, p3, p4):
        p.close()


def test_train_pairs_driver(gpu_device, files, tmp_path):
    root, _ = files
    ckpt = str(tmp_path / "ckpt.pth")
    base = [sys.executable, os.path.join(ROOT, "tools", "train_pairs.py"), "--model", "b32-yfcc-msclips", "--pairs",
            os.path.join(root, "pairs.tsv"), "--root", root, "--epochs", "2", "--batch", "16", "--random-init", "--workers", "8"]

    def losses(text):
        return [float(v) for v in re.findall(r"step\s+\d+\s+loss (\S+)", text)]
    r = subprocess.run(base + ["--steps", "3", "--save", ckpt, "PRINT_FREQ", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    first = losses(r.stdout)
    assert len(first) == 3 and all(np.isfinite(first)) and os.path.exists(ckpt) and os.path.exists(ckpt + ".input.pt")
    order0 = augment.epoch_order(48, 0, 0, 0, 1, 16)
    assert "first batch indices: " + " ".join(str(int(i)) for i in order0[0]) in r.stdout
    r = subprocess.run(base + ["--steps", "2", "--resume", ckpt, "PRINT_FREQ", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    more = losses(r.stdout)
    assert len(more) == 2 and all(np.isfinite(more)) and "step      3  loss" in r.stdout and "step      4  loss" in r.stdout
    # epoch 0 has three batches of 16: the resumed run starts with the first batch of epoch 1, as the uninterrupted order gives it
    order1 = augment.epoch_order(48, 1, 0, 0, 1, 16)
    assert "first batch indices: " + " ".join(str(int(i)) for i in order1[0]) in r.stdout
