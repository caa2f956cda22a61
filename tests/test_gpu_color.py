"""The colour stage on the GPU: msclip_color_augment (include/msclip_color.h) against the numpy restatement of tests/color_ref.py,
BITWISE (out_u8 and out, fp32 and bf16): every operation is a correctly rounded IEEE operation or integer arithmetic and the blur
weights are data, so a difference is a bug, not a tolerance.  Then the `stages` subsets, repeatability, the all-off identity, the
wrapper's refusals, and msclip_amd.pairs.PairPipeline with the colour stage on (content, replay, resume) and off (today's bits)."""
import numpy as np
import pytest
import torch

import augment_ref as A
import color_ref as C
from msclip_amd import augment, color_hip, input_hip, pairs, zeroshot
from msclip_amd._decode_worker import load_source
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu

SHAPES = ((6, 7, 5), (6, 16, 16), (6, 33, 20), (6, 64, 64), (2, 224, 224))      # (B, H, W)
_CASE = {}


def _case(shape):
    """(src, ops, coef, the restatement's out_u8 at stages 7) of a shape, computed once."""
    if shape not in _CASE:
        B, H, W = shape
        src, ops, coef = C.batch6(H, W)
        if B == 2:                                       # contrast in the middle + hue + gray + blur | contrast last + blur
            src, ops, coef = src[[1, 2]], ops[[1, 2]].copy(), coef[[1, 2]]
            ops[0, 6] = 1
        _CASE[shape] = (src, ops, coef, C.augment_u8(src, ops, coef, 7))
    return _CASE[shape]


def _lut_np():
    return np.ascontiguousarray(np.random.RandomState(0).randn(3, 256).astype(np.float32))


def _run(dev, src, ops, coef, stages=7, bf16=False):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    out, u8 = color_hip.color_augment(t(src), t(ops), t(coef), t(_lut_np()), stages=stages, bf16=bf16, want_u8=True)
    torch.cuda.synchronize()
    return out, u8


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_color_augment_bitwise(gpu_device, shape):
    src, ops, coef, want = _case(shape)
    out, u8 = _run(gpu_device, src, ops, coef)
    got = u8.cpu().numpy()
    diff = np.argwhere(got != want)
    print(f"{shape}: {len(diff)} of {got.size} values differ from the restatement")
    assert len(diff) == 0, diff[:8]
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), C.lookup(want, _lut_np()))
    outb, u8b = _run(gpu_device, src, ops, coef, bf16=True)
    assert outb.dtype == torch.bfloat16 and torch.equal(u8b, u8) and torch.equal(outb, out.to(torch.bfloat16))
    out2, u82 = _run(gpu_device, src, ops, coef)                             # a second call is bitwise the first
    assert torch.equal(u82, u8) and torch.equal(out2, out)


@pytest.mark.parametrize("stages", (1, 2, 4, 7, 0, 3, 5, 6))
def test_stages_subsets(gpu_device, stages):
    """A launch that provides for a subset of the stages agrees with the full launch on images whose other flags are off, and
    with the restatement under that mask on images whose other flags are on (a clear bit turns the stage off)."""
    src, ops, coef = C.batch6(33, 20, seed=1)
    _, u8 = _run(gpu_device, src, ops, coef, stages)
    assert np.array_equal(u8.cpu().numpy(), C.augment_u8(src, ops, coef, stages))
    masked = ops.copy()
    if not stages & 1:
        masked[:, :4] = -1
    if not stages & 2:
        masked[:, 5] = 0
    if not stages & 4:
        masked[:, 6] = 0
    _, full = _run(gpu_device, src, masked, coef, 7)
    assert torch.equal(u8, full)


def test_all_flags_off_is_the_table(gpu_device):
    src, ops, coef = C.batch6(33, 20, seed=2)
    ops[:] = [-1, -1, -1, -1, 77, 0, 0, 0]
    lut = torch.from_numpy(_lut_np()).to(gpu_device)
    for stages in (7, 0):
        out, u8 = _run(gpu_device, src, ops, coef, stages)
        s = torch.from_numpy(src).to(gpu_device)
        assert torch.equal(u8, s) and torch.equal(out, torch.stack([lut[c][s[..., c].long()] for c in range(3)], dim=1))


def test_color_augment_wrapper_refuses(gpu_device):
    dev = gpu_device
    src = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    ops, coef = torch.zeros(2, 8, dtype=torch.int32, device=dev), torch.zeros(2, 12, device=dev)
    lut = torch.zeros(3, 256, device=dev)
    for bad in (dict(src=src.float()), dict(src=src[..., :2]), dict(ops=ops.long()), dict(ops=ops[:1]), dict(coef=coef[:, :11]),
                dict(coef=coef.double()), dict(lut=lut[:2]), dict(stages=8), dict(stages=-1), dict(stages=True), dict(src=src.cpu()),
                dict(src=src[:0]), dict(out=torch.zeros(2, 3, 16, 16, dtype=torch.bfloat16, device=dev)),
                dict(src=torch.zeros(1, 4, 631, 3, dtype=torch.uint8, device=dev), ops=ops[:1], coef=coef[:1])):
        args = dict(src=src, ops=ops, coef=coef, lut=lut, stages=7)
        args.update(bad)
        with pytest.raises(ValueError):
            color_hip.color_augment(args.pop("src"), args.pop("ops"), args.pop("coef"), args.pop("lut"), **args)


# ---------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return A.make_files(str(tmp_path_factory.mktemp("pairs_colour")), n=32)


@pytest.fixture(scope="module")
def tokenizer():
    from msclip_amd.tokenizer import SimpleTokenizer
    return SimpleTokenizer()


COLOUR = ["AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 0.8]", "AUG.GRAY_SCALE", "0.2", "AUG.GAUSSIAN_BLUR", "0.5", "AUG.FLIP_PROB", "0.5"]


def test_pipeline_with_colour(gpu_device, files, tokenizer):
    dev = gpu_device
    settings = dict(augment.aug_settings(named_config("b32-yfcc-msclips", COLOUR), colour=True), size=64)
    assert augment.colour_stages(settings) == 7
    lut = zeroshot.normalise_lut(settings["mean"], settings["std"])

    def run(pipe, n=None):
        got = []
        for img, tok, index in pipe:
            got.append((img.clone(), tok.clone(), index.clone(), pipe.last_boxes.clone(), pipe.last_ops.clone(), pipe.last_coef.clone()))
            if n is not None and len(got) == n:
                break
        return got

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    p1 = pairs.PairPipeline(files, 8, dev, settings, tokenizer=tokenizer, seed=5, workers=8, slot=256)
    first, seen = [], {"jitter": 0, "gray": 0, "blur": 0}
    for img, tok, index in p1:
        assert img.dtype == torch.float32 and tuple(img.shape) == (8, 3, 64, 64)
        src = torch.zeros(8, 256, 256, 3, dtype=torch.uint8)
        for j, i in enumerate(index.tolist()):
            a = load_source(files[i][0], 256)
            src[j, :a.shape[0], :a.shape[1]] = torch.from_numpy(a)
        _, u8 = input_hip.resized_crop(src.to(dev), p1.last_dims.to(dev), p1.last_boxes.to(dev), lut.to(dev), 64,
                                       flip=p1.last_flip.to(dev), filter=settings["interpolation"], want_u8=True)
        ops, coef = p1.last_ops, p1.last_coef
        assert ops.dtype == torch.int32 and tuple(ops.shape) == (8, 8) and coef.dtype == torch.float32 and tuple(coef.shape) == (8, 12)
        want = C.lookup(C.augment_u8(u8.cpu().numpy(), ops.numpy(), coef.numpy(), 7), lut.numpy())
        assert np.array_equal(img.cpu().numpy(), want)
        seen["jitter"] += int((ops[:, :4] >= 0).any(dim=1).sum())
        seen["gray"] += int((ops[:, 5] != 0).sum())
        seen["blur"] += int((ops[:, 6] != 0).sum())
        first.append((img.clone(), tok.clone(), index.clone(), p1.last_boxes.clone(), ops.clone(), coef.clone()))
    assert len(first) == 4 and all(0 < v < 32 for v in seen.values()), seen
    # replay: the same seed gives the same batches; resume: the state after batch 1 continues with batch 2
    p2 = pairs.PairPipeline(files, 8, dev, settings, tokenizer=tokenizer, seed=5, workers=3, slot=256)
    head = run(p2, 2)
    assert same(head, first[:2])
    state = p2.state_dict()
    p3 = pairs.PairPipeline(files, 8, dev, settings, tokenizer=tokenizer, seed=77, workers=8, slot=256)
    p3.load_state_dict(state)
    assert same(run(p3), first[2:]) and same(run(p2), first[2:])
    for p in (p1, p2, p3):
        p.close()


def test_pipeline_colour_off_is_unchanged(gpu_device, files, tokenizer):
    """With every colour switch off, a pipeline built from aug_settings(colour=True) yields bitwise what one built from the plain
    settings dict yields: the same draws, the same launch."""
    cfg = named_config("b32-yfcc-msclips", ["AUG.FLIP_PROB", "0.5"])
    plain = dict(augment.aug_settings(cfg), size=64)
    off = dict(augment.aug_settings(cfg, colour=True), size=64)
    assert augment.colour_stages(off) == 0 and augment.colour_stages(plain) == 0
    got = []
    for settings in (plain, off):
        pipe = pairs.PairPipeline(files, 8, gpu_device, settings, tokenizer=tokenizer, seed=5, workers=8, slot=256)
        assert pipe.stages == 0
        got.append([(img.clone(), tok.clone(), index.clone(), pipe.last_boxes.clone(), pipe.last_flip.clone()) for img, tok, index in pipe])
        assert pipe.last_ops is None and pipe.last_coef is None
        state = pipe.state_dict()
        pipe.close()
        got[-1].append((state["rng_state"],))
    assert len(got[0]) == 5 and all(torch.equal(x, y) for p, q in zip(*got) for x, y in zip(p, q))
