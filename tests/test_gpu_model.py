"""End-to-end parity of the HIP path (bf16 operands, fp32 accumulation/residual) on a real MI355X:
against the golden vectors captured from the reference, against the CPU oracle on other seeds / ragged batches,
and through size-independent properties at the benchmark's full batch.

Stated tolerance for bf16 vs the fp32 reference: unit-norm features max-abs <= 5e-3 and
cosine >= 0.9999; logits (T = 1/0.07) max-abs <= 0.05; the reference's own CPU bf16-autocast run differs from
its fp32 run by 1.2e-3 / cos 0.99998."""
import numpy as np
import pytest
import torch

from conftest import golden, set_opt, synth_sd
from msclip_amd import hip, synth
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O

pytestmark = pytest.mark.gpu
FEAT_TOL, COS_TOL, LOGIT_TOL = 5e-3, 0.9999, 0.05
_MODELS = {}


def model_for(name):
    if name not in _MODELS:
        m = get_clip_model(named_config(name))
        m.load_state_dict(synth_sd(name), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


def check_feats(got, ref):
    got, ref = got.float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1).min().item()
    assert err <= FEAT_TOL and cos >= COS_TOL, f"max-abs {err:.3e}, min cos {cos:.6f}"
    return err, cos


@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "b16-yfcc-msclips"])
def test_against_reference_golden(gpu_device, name):
    g = golden(name)
    m = model_for(name)
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    ei, ci = check_feats(m.encode_image(img), g["image_features"])
    et, ct = check_feats(m.encode_text(tok), g["text_features"])
    logits = m(img, tok).cpu()
    assert logits.shape == (b, b)
    el = np.abs(logits.numpy() - g["logits"]).max()
    print(f"{name}: observed margins vs the reference golden: image max-abs {ei:.2e} cos {ci:.6f}; text max-abs {et:.2e} "
          f"cos {ct:.6f}; logits max-abs {el:.2e}  (tolerances {FEAT_TOL} / {COS_TOL} / {LOGIT_TOL})")
    assert el <= LOGIT_TOL
    raw = m.encode_image(img, norm=False).cpu().numpy()
    ref = g["image_features_raw"]
    assert np.abs(raw - ref).max() <= 2e-2 * np.abs(ref).max()
    # the native library really is what ran
    with open("/proc/self/maps") as f:
        assert "libmsclip_hip.so" in f.read()


def test_against_oracle_ragged_batches_and_loss(gpu_device):
    name, arch = "b32-yfcc-msclips", O.arch_b32()
    m, sd = model_for(name), synth_sd(name)
    img = synth.synth_images(3, seed=21)
    tok = synth.synth_tokens(5, seed=22, min_len=1, max_len=75)
    tok[0, :] = 0
    tok[0, 0], tok[0, 1] = 49406, 49407                              # shortest caption: EOT at position 1
    with torch.no_grad():
        ri, rt = O.encode_image(img, sd, arch), O.encode_text(tok, sd, arch)
    check_feats(m.encode_image(img.cuda()), ri)
    check_feats(m.encode_text(tok.cuda()), rt)
    # joint run (towers batched through the shared layers) must agree with the separate runs
    with torch.no_grad():
        ri5 = O.encode_image(synth.synth_images(5, seed=23), sd, arch)
    w = m.engine().run(synth.synth_images(5, seed=23).cuda(), tok.cuda())
    check_feats(w["fv"], ri5)
    check_feats(w["ft"], rt)
    lg = m(synth.synth_images(5, seed=23).cuda(), tok.cuda()).cpu()
    ref_lg = O.clip_logits(ri5, rt, sd["logit_scale"])
    assert (lg - ref_lg).abs().max() <= LOGIT_TOL
    loss = m.contrastive_loss(synth.synth_images(5, seed=23).cuda(), tok.cuda()).item()
    assert abs(loss - O.contrastive_loss(ref_lg).item()) <= 2e-2
    assert abs(loss - O.contrastive_loss(lg).item()) <= 2e-3          # fused/sharded form == full-matrix form


def test_batch_invariance_and_determinism(gpu_device):
    m = model_for("b32-yfcc-msclips")
    img = synth.synth_images(6, seed=31).cuda()
    a = m.encode_image(img)
    b = m.encode_image(img)
    assert torch.equal(a, b)                                          # no atomics / races: bitwise repeatable
    c = m.encode_image(img[2:3])
    assert (a[2:3] - c).abs().max().item() <= 1e-5                    # per-sample result independent of the batch


@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "b16-yfcc-msclips"])
def test_fused_front_paths_against_the_conv_by_conv_chain(gpu_device, monkeypatch, name):
    """The fused stem pass / fused first bottleneck and the kernel-by-kernel chain they replace give the same image
    features (same bf16 roundings of every tensor that exists in both; the fused block keeps the shortcut in fp32)."""
    m = model_for(name)
    img = synth.synth_images(5, seed=37).cuda()
    fused = m.encode_image(img)
    set_opt(monkeypatch, m, block_unfused=True)
    no_block = m.encode_image(img)
    set_opt(monkeypatch, m, front_unfused=True)
    chain = m.encode_image(img)
    monkeypatch.setenv("MSCLIP_FRONT_4WAVE", "1")
    set_opt(monkeypatch, m, front_unfused=False, block_unfused=True)
    four_wave = m.encode_image(img)
    for other in (no_block, chain, four_wave):
        assert (fused - other).abs().max().item() <= 2e-3
        assert torch.nn.functional.cosine_similarity(fused, other, dim=-1).min().item() >= 0.99995


def test_full_bench_batch_properties(gpu_device):
    """BASELINE config C2 (B = 512): finite, unit-norm, logits = scaled cosine, loss identity, rows match a small run."""
    m = model_for("b32-yfcc-msclips")
    B = 512
    img = synth.synth_images(B, seed=41).cuda()
    tok = synth.synth_tokens(B, seed=42).cuda()
    w = m.engine().run(img, tok)
    fi, ft = w["fv"].clone(), w["ft"].clone()
    assert torch.isfinite(fi).all() and torch.isfinite(ft).all()
    assert (fi.norm(dim=-1) - 1).abs().max().item() < 1e-4 and (ft.norm(dim=-1) - 1).abs().max().item() < 1e-4
    lg = m(img, tok)
    ref = m.engine().logit_scale_exp * fi @ ft.t()
    assert (lg - ref).abs().max().item() <= 0.05
    loss = m.contrastive_loss(img, tok).item()
    lab = torch.arange(B, device="cuda")
    ce = 0.5 * (torch.nn.functional.cross_entropy(lg, lab) + torch.nn.functional.cross_entropy(lg.t(), lab)).item()
    assert abs(loss - ce) <= 2e-3
    small_i = m.encode_image(img[100:104])
    small_t = m.encode_text(tok[300:303])
    # the small run goes through other tile configurations (fp32 sums associate differently -> bf16 rounding flips)
    assert (small_i - fi[100:104]).abs().max().item() <= 2e-3
    assert (small_t - ft[300:303]).abs().max().item() <= 2e-3
    # and the full-size path (large-tile kernels everywhere) is pinned to the oracle on a few of its samples
    sd, arch = synth_sd("b32-yfcc-msclips"), O.arch_b32()
    with torch.no_grad():
        ri, rt = O.encode_image(img[[0, 255, 511]].cpu(), sd, arch), O.encode_text(tok[[1, 256, 510]].cpu(), sd, arch)
    check_feats(fi[[0, 255, 511]], ri)
    check_feats(ft[[1, 256, 510]], rt)
    # single-tower calls at the same size (other row counts -> other tile grids)
    check_feats(m.encode_image(img)[[0, 255, 511]], ri)
    check_feats(m.encode_text(tok)[[1, 256, 510]], rt)


def test_full_batch_b16_against_oracle(gpu_device):
    """BASELINE config C3 (ViT-B/16, B = 256: 197-token attention, 14 x 14 adapters) against the oracle on a few samples."""
    name = "b16-yfcc-msclips"
    m, sd, arch = model_for(name), synth_sd(name), O.arch_b16()
    B = 256
    img = synth.synth_images(B, seed=43).cuda()
    tok = synth.synth_tokens(B, seed=44).cuda()
    w = m.engine().run(img, tok)
    fi, ft = w["fv"].clone(), w["ft"].clone()
    assert torch.isfinite(fi).all() and torch.isfinite(ft).all()
    with torch.no_grad():
        check_feats(fi[[0, 128, 255]], O.encode_image(img[[0, 128, 255]].cpu(), sd, arch))
        check_feats(ft[[2, 100, 254]], O.encode_text(tok[[2, 100, 254]].cpu(), sd, arch))


def test_inputs_validated(gpu_device):
    m = model_for("b32-yfcc-msclips")
    with pytest.raises(ValueError):
        m.encode_image(torch.zeros(1, 3, 128, 128, device="cuda"))
    with pytest.raises(ValueError):
        m.encode_text(torch.zeros(1, 60, dtype=torch.long, device="cuda"))
    with pytest.raises(hip.HipUnavailable):
        m.encode_text(torch.zeros(1, 77, dtype=torch.long))


def test_zeroshot_pipeline_against_oracle(gpu_device, tmp_path):
    """BASELINE config C1 plumbing (zero-shot driver) on generated images: classifier columns, 100*f@W logits and
    the top-1 decisions must follow the oracle's (reference tools/zero_shot.py:122-134, 265-266)."""
    import zlib
    from PIL import Image
    from msclip_amd import zeroshot
    name, arch = "b32-yfcc-msclips", O.arch_b32()
    m, sd = model_for(name), synth_sd(name)

    class FakeTok:                                       # deterministic stand-in for the BPE (vocab file not on this box)
        def __call__(self, texts, context_length=77):
            if isinstance(texts, str):
                texts = [texts]
            out = torch.zeros(len(texts), context_length, dtype=torch.long)
            for i, t in enumerate(texts):
                r = np.random.default_rng(zlib.crc32(t.encode()))
                n = int(r.integers(3, 20))
                out[i, 0], out[i, 1:1 + n], out[i, 1 + n] = 49406, torch.from_numpy(r.integers(1, 49000, n)), 49407
            return out

    tok = FakeTok()
    classes = ["tench", "goldfish", "shark"]
    templates = ["a photo of a {}.", "a bad photo of a {}.", "art of the {}.", "itap of a {}."]
    W = zeroshot.zeroshot_classifier(m, tok, classes, templates, classes_per_batch=2)
    with torch.no_grad():
        Wref = O.zeroshot_classifier([tok([t.format(c) for t in templates]) for c in classes], sd, arch)
    assert W.shape == (512, 3) and (W.float().cpu() - Wref).abs().max().item() <= FEAT_TOL
    rng = np.random.default_rng(5)
    for ci, c in enumerate(["n01", "n02", "n03"]):
        (tmp_path / "val" / c).mkdir(parents=True)
        for k in range(3):
            Image.fromarray(rng.integers(0, 256, (240 + 10 * k, 260, 3), dtype=np.uint8)).save(tmp_path / "val" / c / f"{k}.png")
    res = zeroshot.evaluate(m, tok, str(tmp_path / "val"), classes, templates, batch_size=4, log=lambda s: None)
    assert res["n"] == 9 and 0.0 <= res["top1"] <= 100.0
    _, items = zeroshot.image_folder(str(tmp_path / "val"))
    x = torch.stack([zeroshot.preprocess(Image.open(p)) for p, _ in items])
    with torch.no_grad():
        ref_logits = 100.0 * O.encode_image(x, sd, arch) @ Wref
    got_logits = 100.0 * m.encode_image(x.cuda()).float().cpu() @ W.float().cpu()
    assert (got_logits - ref_logits).abs().max().item() <= 0.3        # stated zero-shot logit tolerance (x100 scale)
    y = torch.tensor([c for _, c in items])
    assert abs(res["top1"] - zeroshot.accuracy(ref_logits, y)[0]) <= 100.0 / 9 + 1e-6


def test_hipgraph_replay_matches_eager(gpu_device):
    m = model_for("b32-yfcc-msclips")
    eng = m.engine()
    img = synth.synth_images(4, seed=61).cuda()
    tok = synth.synth_tokens(4, seed=62).cuda()
    w = eng.run(img, tok)
    fi, ft = w["fv"].clone(), w["ft"].clone()
    replay = eng.graph(4, 4)
    w2 = replay(img, tok)
    assert torch.equal(w2["fv"], fi) and torch.equal(w2["ft"], ft)          # same kernels, same order: bitwise equal
    img2 = synth.synth_images(4, seed=63).cuda()
    w3 = replay(img2, tok)
    assert torch.equal(w3["fv"], eng.run(img2, tok)["fv"])
    only_txt = eng.graph(0, 80)
    t80 = synth.synth_tokens(80, seed=64).cuda()
    assert torch.equal(only_txt(tok=t80)["ft"], eng.run(tok=t80)["ft"])


# ---------------------------------------------------------------------------------------------------------------------
# round 2: BASELINE config C4's per-rank workload, the emulated 8-rank contrastive head, reference taps, real tokens, C1
# ---------------------------------------------------------------------------------------------------------------------

def test_c4_per_rank_batch_1024_against_oracle(gpu_device):
    """BASELINE config C4, one rank's share: ViT-B/32 towers at per-GPU batch 1024 (130 048 token rows per projection
    GEMM, other tile grids than B = 512) pinned to the oracle on sampled rows of both towers."""
    name, arch = "b32-yfcc-msclips", O.arch_b32()
    m, sd = model_for(name), synth_sd(name)
    B = 1024
    img = synth.synth_images(B, seed=71).cuda()
    tok = synth.synth_tokens(B, seed=72).cuda()
    w = m.engine().run(img, tok)
    fi, ft = w["fv"].clone(), w["ft"].clone()
    assert torch.isfinite(fi).all() and torch.isfinite(ft).all()
    assert (fi.norm(dim=-1) - 1).abs().max().item() < 1e-4 and (ft.norm(dim=-1) - 1).abs().max().item() < 1e-4
    si, st = [0, 511, 512, 1023], [1, 300, 777, 1022]
    with torch.no_grad():
        ei, ci = check_feats(fi[si], O.encode_image(img[si].cpu(), sd, arch))
        et, ct = check_feats(ft[st], O.encode_text(tok[st].cpu(), sd, arch))
    print(f"C4 per-rank B=1024: image max-abs {ei:.2e} cos {ci:.6f}; text max-abs {et:.2e} cos {ct:.6f}")


def test_emulated_8_rank_contrastive_head(gpu_device):
    """BASELINE config C4's head on one GPU: eight local batches of 1024 stand for the eight ranks; every "rank" gets
    the rank-major concatenation as the gathered operands and its label offset rank * B (reference lib/utils/comm.py:
    150-153).  The per-rank shares (engine.loss_from_features = what forward_loss computes before its all-reduce) must
    equal the rows / columns of that rank in the full 8192 x 8192 symmetric CE the oracle forms from the same features,
    and their sum the oracle's loss."""
    m = model_for("b32-yfcc-msclips")
    eng = m.engine()
    B, W = 1024, 8
    loc_i, loc_t = [], []
    for r in range(W):
        w = eng.run(synth.synth_images(B, seed=200 + r).cuda(), synth.synth_tokens(B, seed=300 + r).cuda())
        loc_i.append(w["fvb"].clone())
        loc_t.append(w["ftb"].clone())
    all_i, all_t = torch.cat(loc_i), torch.cat(loc_t)                       # rank-major, like gather_tensors
    logits = (eng.logit_scale_exp * all_i.float() @ all_t.float().t()).cpu()     # the checker's full N x N matrix
    n = W * B
    ref_total = O.contrastive_loss(logits).item()
    lse_r, lse_c, diag = torch.logsumexp(logits, 1), torch.logsumexp(logits, 0), logits.diag()
    shares = []
    for r in range(W):
        s = eng.loss_from_features(loc_i[r], loc_t[r], all_i, all_t, r * B).item()
        rows = slice(r * B, (r + 1) * B)
        ref = ((lse_r[rows] - diag[rows]).sum() + (lse_c[rows] - diag[rows]).sum()).item() / (2 * n)
        assert abs(s - ref) <= 2e-4 * max(1.0, abs(ref)), (r, s, ref)
        shares.append(s)
    assert abs(sum(shares) - ref_total) <= 5e-4, (sum(shares), ref_total)
    with pytest.raises(AssertionError):
        eng.loss_from_features(loc_i[0], loc_t[0], all_i, all_t, n)         # label offset outside the gathered batch


TAP_TOL = {"stem": 3e-2, "parallel": 3e-2, "tokens": 3e-2, "adapter": 3e-2, "vblock": 4e-2, "tblock": 4e-2}


def _live_sample_mask(shape, lens):
    """Which of summarize()'s 64 strided sample points of a [B, L, C] text tap lie on live rows (l < lens[b])."""
    n = int(np.prod(shape))
    idx = torch.linspace(0, n - 1, 64).long().clamp_(max=n - 1)
    row = idx // shape[2]
    b, l = row // shape[1], row % shape[1]
    return (l < lens.cpu().long()[b]).numpy()


@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "b16-yfcc-msclips"])
@pytest.mark.parametrize("fused,pack", [(True, True), (False, True), (True, False)])
def test_reference_taps_on_gpu(gpu_device, monkeypatch, name, fused, pack):
    """Every intermediate the reference exposes through forward hooks (tests/golden tap_*: stem stages, parallel
    stages 0-4, tokens after ln_pre, lateral adapters 0-4, blocks 1 / 2 / 11 of both towers), HIP path vs the values
    captured from the REAL reference: a compensating error in the stem / adapter kernels cannot hide behind the end
    features.  Compared on the golden's 64-point strided sample + mean + abs-mean, relative to the tap's own scale
    (bf16 activations: 3e-2 of the sample's abs-max; blocks 4e-2).  pack: the text rows packed (default; the text-block taps
    then exist on the live rows only: their sample points on live rows are compared, the whole-tensor means are not) or all
    77 rows per caption (MSCLIP_TEXT_PACK=0: the complete comparison)."""
    from conftest import summarize
    g = golden(name)
    m = model_for(name)
    set_opt(monkeypatch, m, text_pack=bool(pack))
    if not fused:
        set_opt(monkeypatch, m, front_unfused=True, block_unfused=True)
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    taps = {}
    m.engine().run(img, tok, taps=taps)
    names = [k[4:] for k in g.files if k.startswith("tap_")]
    assert len(names) == 23
    checked, worst = 0, {}
    for k in names:
        if k == "stem_out":
            continue                                   # last_conv's output only exists fused with +pos / scatter: tokens_ln_pre covers it
        if k == "stem_conv1" and fused:
            continue                                   # conv1's map never leaves the chip on the fused path
        assert k in taps, k
        t = taps[k]
        assert tuple(t.shape) == tuple(g["tapshape_" + k]), (k, t.shape, g["tapshape_" + k])
        got, ref = summarize(t), g["tap_" + k]
        scale = max(np.abs(ref[2:]).max(), 1e-3)
        tol = TAP_TOL[[p for p in TAP_TOL if k.startswith(p)][0]]
        if k.startswith("tblock") and pack:
            assert "text_lengths" in taps
            live = _live_sample_mask(t.shape, taps["text_lengths"])
            assert live.sum() >= 16, (k, live.sum())
            err = np.abs(got[2:] - ref[2:])[live].max() / scale
            assert bool((got[2:][~live] == 0).all())
        else:
            err = np.abs(got[2:] - ref[2:]).max() / scale
            assert abs(got[0] - ref[0]) <= tol * max(ref[1], 1e-3) and abs(got[1] - ref[1]) <= tol * max(ref[1], 1e-3), (k, got[:2], ref[:2])
        worst[k] = float(err)
        assert err <= tol, (k, err)
        checked += 1
    assert checked == (21 if fused else 22)
    print(name, "fused" if fused else "unfused", "worst taps:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])


def _c1_folder(root):
    """The generated 64-image ImageFolder of BASELINE config C1 (same generator as tools/make_golden.py::c1_images)."""
    from PIL import Image
    rng = np.random.default_rng(7)
    low = rng.integers(0, 256, (8, 8, 14, 14, 3)).astype(np.float32)
    img = np.repeat(np.repeat(low, 16, axis=2), 16, axis=3)
    img += rng.normal(0, 12, img.shape).astype(np.float32)
    img = np.clip(img, 0, 255).astype(np.uint8)
    for c in range(8):
        d = root / "val" / f"n{c:08d}"
        d.mkdir(parents=True)
        for k in range(8):
            Image.fromarray(img[c, k]).save(d / f"{k}.png")


def test_real_tokens_and_c1_zeroshot_cli_against_reference(gpu_device, tmp_path):
    """BASELINE config C1 end to end with REAL CLIP token ids, against values captured from the reference
    (tests/golden/b32-yfcc-msclips.zeroshot.npz, tools/make_golden.py::zeroshot_fixture):
    (1) the committed token ids of tests/golden/tokenizer.json through the HIP text tower;
    (2) tools/eval_zeroshot.py's command line (--ds imagenet --model yaml KEY VALUE..., double update_config, strict
        checkpoint load from a file, packaged BPE merges + ImageNet prompts, generated 64-image ImageFolder):
        classifier columns of 8 classes x 80 templates, 100 * f @ W logits, top-1."""
    import json
    import os
    import sys
    from conftest import GOLDEN, ROOT
    from msclip_amd import checkpoint
    z = np.load(os.path.join(GOLDEN, "b32-yfcc-msclips.zeroshot.npz"))
    name = "b32-yfcc-msclips"
    m = model_for(name)
    ids = torch.tensor(json.load(open(os.path.join(GOLDEN, "tokenizer.json")))["ids"], dtype=torch.long)
    check_feats(m.encode_text(ids.cuda()), z["prompt_text_features"])
    # --- the CLI
    _c1_folder(tmp_path)
    ckpt = tmp_path / "synth_ckpt.pth"
    torch.save(synth_sd(name), ckpt)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_zeroshot as E
    args = E.parse_args(["--ds", "imagenet", "--model", os.path.join(ROOT, "experiments", "model", name + ".yaml"),
                         "--max-classes", "8", "DATASET.ROOT", str(tmp_path), "MODEL.PRETRAINED_MODEL", str(ckpt),
                         "TEST.BATCH_SIZE_PER_GPU", "16"])
    cfg = E.build_config(E.resolve_dataset("imagenet"), args.model, args.opts)
    assert cfg.NAME == "" and cfg.DATASET.DATASET == "imagenet" and cfg.TEST.METRIC == "accuracy"
    lines = []
    from msclip_amd import zeroshot
    real_eval = zeroshot.evaluate
    out = {}

    def spy(*a, **k):
        out.update(real_eval(*a, return_logits=True, **k))
        return out
    zeroshot.evaluate = spy
    try:
        res = E.zero_shot(args, E.resolve_dataset("imagenet"), log=lines.append)
    finally:
        zeroshot.evaluate = real_eval
    assert res["n"] == 64
    assert (out["classifier"] - torch.from_numpy(z["classifier"])).abs().max().item() <= FEAT_TOL
    assert (out["logits"] - torch.from_numpy(z["logits"])).abs().max().item() <= 0.3          # stated x100 tolerance
    agree = (out["logits"].argmax(-1) == torch.from_numpy(z["logits"]).argmax(-1)).float().mean().item()
    assert agree >= 0.95, agree
    assert abs(res["top1"] - float(z["top1"])) <= 100.0 * 3 / 64 + 1e-6
    assert any(s.startswith("=> imagenet% TEST:") and "accuracy@1" in s for s in lines)
    assert any("load model file" in s for s in lines)


def test_engine_repacks_after_in_place_weight_changes(gpu_device):
    """The packed bf16 copies follow the module: submodule load_state_dict, logit_scale.fill_, param.copy_ (mutations
    the CLIP-level hooks cannot see) are picked up at the next call; a captured hipGraph refuses to replay stale weights."""
    name = "b32-yfcc-msclips"
    m = get_clip_model(named_config(name))
    m.load_state_dict(synth_sd(name), strict=True)
    m = m.cuda().eval()
    img = synth.synth_images(2, seed=81).cuda()
    tok = synth.synth_tokens(2, seed=82).cuda()
    f0, l0 = m.encode_image(img), m(img, tok)
    with torch.no_grad():
        m.logit_scale.fill_(1.0)
    l1 = m(img, tok)
    ratio = (l1 / l0).flatten()
    expect = float(torch.tensor(1.0).exp() / synth_sd(name)["logit_scale"].exp())
    assert (ratio - expect).abs().max().item() <= 1e-3 * expect
    replay = m.engine().graph(2, 0)
    replay(img=img)
    with torch.no_grad():
        m.visual.proj.mul_(-1.0)
    f1 = m.encode_image(img)
    assert (f1 + f0).abs().max().item() <= 1e-6                              # sign flip of the projection seen
    with pytest.raises(RuntimeError, match="changed after this hipGraph"):
        replay(img=img)
    vis = {k: v for k, v in synth_sd(name).items() if k.startswith("visual.")}
    m.visual.load_state_dict({k[len("visual."):]: v for k, v in vis.items()})
    assert torch.equal(m.encode_image(img), f0)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs of one node (the RCCL all-gather path at N > 1)")
def test_two_rank_rccl_gather_matches_single_process(gpu_device, tmp_path):
    """forward (full N x N logits after the rank-major RCCL all-gather) and forward_loss (local row / column blocks +
    scalar all-reduce) under two ranks against ONE process running the concatenated batch."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = tmp_path / "r0.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29611",
                        os.path.join(ROOT, "tests", "_nccl_worker.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out)
    m = model_for("b32-yfcc-msclips")
    img, tok = synth.synth_images(12, seed=91).cuda(), synth.synth_tokens(12, seed=92).cuda()
    ref_logits = m(img, tok).cpu()
    ref_loss = float(m.contrastive_loss(img, tok))
    assert got["logits"].shape == (12, 12)
    assert (got["logits"] - ref_logits).abs().max().item() <= 2e-2          # per-rank batch 6 vs 12: other tile grids
    assert abs(got["loss"] - ref_loss) <= 2e-3


def test_one_rank_rccl_collectives(gpu_device, tmp_path):
    """RCCL itself on a one-GPU box: a world of ONE rank over the `nccl` backend runs every collective of the N > 1 path
    through librccl (communicator creation, `all_gather_into_tensor` of the features from the side stream, the scalar
    all-reduce of the sharded loss, the bucketed async gradient all-reduce) -- with one rank they are identities, so the
    results must equal the plain single-process run on the same batch."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from msclip_amd import train
    out = tmp_path / "r0.pt"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29617",
                        os.path.join(ROOT, "tests", "_nccl_worker.py"), str(out), "nccl"], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out)
    m = model_for("b32-yfcc-msclips")
    img, tok = synth.synth_images(6, seed=91).cuda(), synth.synth_tokens(6, seed=92).cuda()
    assert torch.equal(got["logits"], m(img, tok).cpu())
    assert got["loss"] == float(m.contrastive_loss(img, tok))
    # the single packed [B, 2, E] gather (MSCLIP_GATHER_PACKED=1): same features through strided views of one buffer
    assert torch.equal(got["logits_packed_gather"], got["logits"]) and got["loss_packed_gather"] == got["loss"]
    # RCCL behind the C ABI (msclip_comm_init / msclip_allgather_feats / msclip_allreduce) against ProcessGroupNCCL: bitwise, eager
    # and as entries of a launch-plan replay (batch 256)
    nat = got["native"]
    assert torch.equal(nat["logits"], got["logits"]) and nat["loss"] == got["loss"]
    assert nat["planned"] and nat["equal256"]
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    assert got["train_loss"] == float(ts.forward(img, tok))
    full = ts.backward()
    assert got["n_grads"] == len(full) and got["launched"] >= 8
    for k, g in got["grads"].items():
        if k == "token_embedding.weight":                              # atomics: order-dependent last bits
            assert torch.allclose(g, full[k].float().cpu(), rtol=1e-3, atol=1e-6), k
        else:
            assert torch.equal(g, full[k].float().cpu()), k


def test_two_one_rank_rccl_processes_share_the_gpu(gpu_device, tmp_path):
    """Two independent processes, each with its own ONE-rank RCCL communicator, run the full N > 1 code path (side-stream
    feature gathers, sharded loss + all-reduce, bucketed gradient all-reduce, AdamW on the reducer's views, a second
    forward / backward) at the same time on GPU 0: two live communicators, their streams and the engine's side / lane
    streams interleaved by the hardware scheduler -- the closest thing to peers a one-GPU box offers.  Both must reproduce
    the single-communicator results bit for bit (each is an identity collective), and each other."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs, outs = [], []
    for i, port in enumerate((29631, 29632)):
        out = tmp_path / f"p{i}.pt"
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                                       "--master-addr", "127.0.0.1", "--master-port", str(port),
                                       os.path.join(ROOT, "tests", "_nccl_worker.py"), str(out), "nccl"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        try:
            _, err = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        assert p.returncode == 0, err[-3000:]
    a, b = torch.load(outs[0]), torch.load(outs[1])
    assert torch.equal(a["logits"], b["logits"]) and a["loss"] == b["loss"] and a["train_loss"] == b["train_loss"]
    assert a["launched"] >= 8 and a["n_grads"] == b["n_grads"]
    for k in a["grads"]:
        if k == "token_embedding.weight":
            assert torch.allclose(a["grads"][k], b["grads"][k], rtol=1e-3, atol=1e-6), k
        else:
            assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert abs(a["train_loss_after_step"] - b["train_loss_after_step"]) <= 1e-5      # (embedding-gradient atomics: last bits)
    assert a["train_loss_after_step"] != a["train_loss"]                              # the step reached the engine's packed copies
    m = model_for("b32-yfcc-msclips")
    img, tok = synth.synth_images(6, seed=91).cuda(), synth.synth_tokens(6, seed=92).cuda()
    assert torch.equal(a["logits"], m(img, tok).cpu())


def test_two_ranks_on_one_gpu_over_gloo(gpu_device, tmp_path):
    """The N > 1 path on a one-GPU box: two processes share GPU 0 and talk over gloo, so everything but RCCL itself runs --
    rank-major feature gathers issued from the side stream, label offsets, the sharded loss + scalar all-reduce, and the
    training step's bucketed gradient all-reduce.  Against the single-process run on the concatenated batch: same
    logits / loss; the rank-averaged gradients times the world size are the full-batch gradients (each rank differentiates
    the global loss through its local rows only, lib/utils/comm.py:151-152)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from msclip_amd import train
    out = tmp_path / "r0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29613",
                        os.path.join(ROOT, "tests", "_nccl_worker.py"), str(out), "gloo"], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out)
    m = model_for("b32-yfcc-msclips")
    img, tok = synth.synth_images(12, seed=91).cuda(), synth.synth_tokens(12, seed=92).cuda()
    ref_logits = m(img, tok).cpu()
    ref_loss = float(m.contrastive_loss(img, tok))
    assert (got["logits"] - ref_logits).abs().max().item() <= 2e-2
    assert abs(got["loss"] - ref_loss) <= 2e-3
    assert torch.equal(got["logits_packed_gather"], got["logits"]) and got["loss_packed_gather"] == got["loss"]      # one packed gather == two
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    full_loss = float(ts.forward(img, tok))
    full = ts.backward()
    assert abs(got["train_loss"] - full_loss) <= 2e-3 and got["n_grads"] == len(full) and got["launched"] >= 8
    for k, g in got["grads"].items():
        ref = full[k].float().cpu()
        # logit_scale multiplies the whole logits matrix, which every rank holds in full (reference: all_I @ all_T^T on every
        # rank): its per-rank gradient already is the global one and the DDP average leaves it unchanged
        mul = 1.0 if k == "logit_scale" else 2.0
        err = ((mul * g - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()
        cos = torch.nn.functional.cosine_similarity((mul * g).flatten(), ref.flatten(), dim=0).item()
        assert err <= 6e-2 and cos >= 0.998, (k, err, cos)            # batch 6 + 6 vs 12: other tile grids / split counts


@pytest.mark.parametrize("extra", [[], ["--train"]])
def test_bench_multi_rank_plumbing_on_one_gpu(gpu_device, extra):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one rank per process), with both ranks on GPU 0
    over gloo (MSCLIP_TEST_SHARED_GPU=1): rendezvous, warm-up, barrier-fenced timed region, max over ranks, ONE JSON line
    from rank 0 with the whole-job value."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, MSCLIP_TEST_SHARED_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29615", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8", "--no-pmc", "--no-cpu-baseline"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0 and rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 16 and rec["config"]["gloo_ranks"] == 2 and "rccl_ranks" not in rec["config"]
    assert "TEST_ONLY" in rec["config"]
    assert abs(rec["value"] - 16 * 2 / (rec["ms_per_step"] * 2e-3)) / rec["value"] < 1e-2      # whole-job pairs / max-rank time


@pytest.mark.parametrize("extra", [[], ["--train", "--bn", "frozen"]])
def test_bench_plain_run_dumps_the_last_step(gpu_device, tmp_path, extra):
    """A plain bench.py run (no --full) prints the headline record without the --full measurements, and --dump-outputs writes
    the last timed step's outputs as float32 .npy files: the loss of the record, and the forward step's unit features (or a
    training step's gradient sample)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", str(out)] + extra, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 8 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-2
    assert not {"roofline", "cpu_baseline", "hbm_bound_kernels"} & set(rec)
    files = sorted(os.listdir(out))
    assert files == (["grad_sample.npy", "loss.npy"] if extra else ["image_features.npy", "loss.npy", "text_features.npy"])
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["loss"].shape == (1,) and abs(float(arrays["loss"][0]) - rec["loss"]) <= 1e-4
    if not extra:
        for k in ("image_features", "text_features"):
            assert arrays[k].shape == (8, 512)
            assert np.abs(np.linalg.norm(arrays[k], axis=1) - 1.0).max() <= 1e-3
    else:
        assert arrays["grad_sample"].ndim == 1 and np.abs(arrays["grad_sample"]).max() > 0


def test_conv_branch_on_side_stream_is_bitwise_the_inline_schedule(gpu_device, monkeypatch):
    """The default schedule issues the parallel convolutional branch + the adapters' top-down halves on a side HIP stream
    (they depend on the image only) with one event per adapter; MSCLIP_CONV_SIDE_STREAM=0 runs them inline: same kernels,
    same data, bitwise the same result."""
    m = model_for("b32-yfcc-msclips")
    img = synth.synth_images(6, seed=91).cuda()
    tok = synth.synth_tokens(6, seed=92).cuda()
    set_opt(monkeypatch, m, conv_side_stream=False)
    a = m.engine().run(img, tok)
    fi, ft = a["fv"].clone(), a["ft"].clone()
    set_opt(monkeypatch, m, conv_side_stream=True)
    for _ in range(3):                                                 # back-to-back steps: buffer reuse across steps
        b = m.engine().run(img, tok)
        assert torch.equal(b["fv"], fi) and torch.equal(b["ft"], ft)


@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "b16-yfcc-msclips"])
def test_last_block_on_live_rows_only_matches_the_full_block(gpu_device, monkeypatch, name):
    """After the last block's attention only x[:, 0] (M.py:2685) and the EOT rows (M.py:3057-3060) are read: the engine runs
    out_proj / ln_2 / c_fc / c_proj of that block on those rows (engine._last_block_tail).  Features, logits and loss against
    the same engine with MSCLIP_FULL_LAST_BLOCK=1 (every row, the reference's schedule): same arithmetic per row, another
    GEMM tile shape -- agreement to bf16-operand rounding of the MLP hidden (far inside the stated tolerance, which both
    also meet against the reference goldens in test_against_reference_golden).  Also image-only / text-only calls and
    ragged batch sizes (compact row ranges)."""
    m = model_for(name)
    img = synth.synth_images(5, seed=71).cuda()
    tok = synth.synth_tokens(7, seed=72, min_len=1, max_len=75).cuda()
    set_opt(monkeypatch, m, full_last_block=True)
    fi, ft = m.encode_image(img), m.encode_text(tok)
    lg = m(img, tok[:5])
    loss = m.contrastive_loss(img, tok[:5]).item()
    set_opt(monkeypatch, m, full_last_block=False)
    ci, ct = m.encode_image(img), m.encode_text(tok)
    assert (ci - fi).abs().max().item() <= 1e-3 and (ct - ft).abs().max().item() <= 1e-3
    assert torch.nn.functional.cosine_similarity(ci, fi, dim=-1).min().item() >= 0.99999
    assert torch.nn.functional.cosine_similarity(ct, ft, dim=-1).min().item() >= 0.99999
    assert (m(img, tok[:5]) - lg).abs().max().item() <= 2e-2
    assert abs(m.contrastive_loss(img, tok[:5]).item() - loss) <= 5e-3
    w = m.engine().run(img, tok[:5])
    assert w["XC"].shape[0] == 10 and torch.isfinite(w["XC"]).all()


def test_inference_between_training_forward_and_backward_keeps_the_gradients(gpu_device):
    """The conv side's activations the backward reads live in the engine's workspace: an inference call of the same shape
    between TrainStep.forward and .backward (an eval / logging call) must not overwrite them -- it gets its own workspace."""
    from msclip_amd import train
    m = get_clip_model(named_config("b32-yfcc-msclips"))
    m.load_state_dict(synth_sd("b32-yfcc-msclips"), strict=True)
    m = m.cuda().eval()
    img, tok = synth.synth_images(4, seed=81).cuda(), synth.synth_tokens(4, seed=82).cuda()
    other = synth.synth_images(4, seed=83).cuda()
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    ts.forward(img, tok)
    ref = ts.backward()
    ts.forward(img, tok)
    m.contrastive_loss(other, tok)                    # same shape, other pixels: would overwrite the stem / branch maps
    m.encode_image(other)
    got = ts.backward()
    for k in ("visual.transformer.resblocks.0.conv1.weight", "visual.transformer.parallel_branch_v.2.resnet_stage.conv_0.conv2.weight",
              "visual.transformer.parallel_lateral_adapter.1.top2bottom_pw_conv.conv.weight"):
        assert torch.equal(ref[k], got[k]), k


def _model_with(name, opts):
    m = get_clip_model(named_config(name, opts))
    m.load_state_dict(synth_sd(name), strict=True)
    return m.cuda().eval()


def test_l16_standin_bf16_against_reference_golden(gpu_device):
    """BASELINE config C5's stand-in (experiments/model/l16-fp8-msclips.yaml: ViT-L width / depth / heads on the 14 x 14 grid)
    is a model the reference itself builds from that yaml: its bf16 path here against features / logits captured from the
    REAL reference (tests/golden/l16-fp8-msclips.npz, tools/make_golden.py --l16), same tolerances as the released configs."""
    name = "l16-fp8-msclips"
    g = golden(name)
    m = _model_with(name, ["MODEL.SPEC.PRECISION", "bf16"])
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    ei, ci = check_feats(m.encode_image(img), g["image_features"])
    et, ct = check_feats(m.encode_text(tok), g["text_features"])
    el = np.abs(m(img, tok).cpu().numpy() - g["logits"]).max()
    print(f"{name} bf16: image max-abs {ei:.2e} cos {ci:.6f}; text max-abs {et:.2e} cos {ct:.6f}; logits max-abs {el:.2e}")
    assert el <= LOGIT_TOL


def test_l14_patch_conv_model_bf16_against_reference_golden(gpu_device):
    """BASELINE config C5 proper (experiments/model/l14-fp8-msclips.yaml): ViT-L/14 with the reference's plain patch convolution
    (M.py:2502-2508, 2655-2668), 16 x 16 grid = 257 tokens, attention / MLP shared from block 1, no conv branch.  The reference
    builds it from that yaml: bf16 path here against features, logits and the captured taps (tokens after ln_pre, blocks 0 / 1 /
    23 of both towers) of the REAL reference (tests/golden/l14-fp8-msclips.npz, tools/make_golden.py --l14)."""
    from conftest import summarize
    name = "l14-fp8-msclips"
    g = golden(name)
    m = _model_with(name, ["MODEL.SPEC.PRECISION", "bf16"])
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    ei, ci = check_feats(m.encode_image(img), g["image_features"])
    et, ct = check_feats(m.encode_text(tok), g["text_features"])
    el = np.abs(m(img, tok).cpu().numpy() - g["logits"]).max()
    print(f"{name} bf16: image max-abs {ei:.2e} cos {ci:.6f}; text max-abs {et:.2e} cos {ct:.6f}; logits max-abs {el:.2e}")
    assert el <= LOGIT_TOL
    taps = {}
    m.engine().run(img, tok, taps=taps)
    names = [k[4:] for k in g.files if k.startswith("tap_")]
    assert len(names) == 7
    for k in names:
        t = taps[k]
        assert tuple(t.shape) == tuple(g["tapshape_" + k]), (k, t.shape)
        got, ref = summarize(t), g["tap_" + k]
        scale = max(np.abs(ref[2:]).max(), 1e-3)
        err = np.abs(got[2:] - ref[2:])
        if k.startswith("tblock") and "text_lengths" in taps:        # packed captions: the sample points on live rows
            live = _live_sample_mask(t.shape, taps["text_lengths"])
            assert live.sum() >= 16 and bool((got[2:][~live] == 0).all())
            err = err[live]
        assert err.max() / scale <= 4e-2, k
    # batch 256 (Mv = 257 * 256 rows: the LayerNorm fold and the 257-token attention at full size) against the oracle on a few samples
    sd, arch = synth_sd(name), O.arch_l14()
    B = 256
    img = synth.synth_images(B, seed=61).cuda()
    tok = synth.synth_tokens(B, seed=62).cuda()
    w = m.engine().run(img, tok)
    fi, ft = w["fv"].clone(), w["ft"].clone()
    with torch.no_grad():
        check_feats(fi[[0, 255]], O.encode_image(img[[0, 255]].cpu(), sd, arch))
        check_feats(ft[[1, 254]], O.encode_text(tok[[1, 254]].cpu(), sd, arch))


@pytest.mark.parametrize("precision", ["fp8", "fp8-qkv"])
@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "l16-fp8-msclips"])
def test_fp8_projections_against_the_bf16_path(gpu_device, name, precision):
    """MODEL.SPEC.PRECISION fp8 (c_fc and c_proj on the MX fp8 MFMA: e4m3 LayerNorm output with per-token scales, e4m3 hidden
    matrix with a calibrated static scale, per-channel weight scales) and fp8-qkv (in_proj as well) have no reference
    semantics: PARITY UNPINNED.  Checked against this build's own bf16 path on the same weights (cosine floors below, on the
    unit features) and, through it, loosely against the reference golden."""
    bf = _model_with(name, ["MODEL.SPEC.PRECISION", "bf16"])
    f8 = _model_with(name, ["MODEL.SPEC.PRECISION", precision])
    assert f8.engine().fp8 and not bf.engine().fp8 and f8.engine().fp8_qkv == (precision == "fp8-qkv")
    img, tok = synth.synth_images(6, seed=33).cuda(), synth.synth_tokens(6, seed=34).cuda()
    # calibration of the MLP hidden matrix's static e4m3 scale on one two-modality batch (explicit; c_fc with a bf16 output, c_proj
    # in bf16 while it runs); the measured calls below run c_fc -> e4m3 hidden -> fp8 c_proj wherever the row count is whole tiles
    assert not f8.engine().fp8_calibrated()
    st = f8.engine().calibrate_fp8(synth.synth_images(256, seed=35).cuda(), synth.synth_tokens(256, seed=36).cuda())
    assert f8.engine().fp8_calibrated() and len(st) >= 2 * (f8.engine().n_layers - 1) - 1
    assert all(b["w"].hid_scale is not None for b in f8.engine().tblk[:-1])      # (the last block's tail runs on the live rows, bf16)
    f8.engine().refresh(force=True)                                              # a re-pack keeps the calibration
    assert f8.engine().fp8_state() == st
    big_i, big_t = synth.synth_images(256, seed=37).cuda(), synth.synth_tokens(256, seed=38).cuda()
    cos = torch.nn.functional.cosine_similarity
    cb = cos(f8.encode_text(big_t), bf.encode_text(big_t), dim=-1).min().item()
    ci_b = cos(f8.encode_image(big_i), bf.encode_image(big_i), dim=-1).min().item()
    print(f"{name} {precision}: batch 256 (fp8 c_proj active): min cosine image {ci_b:.5f} text {cb:.5f}")
    ci = cos(f8.encode_image(img), bf.encode_image(img), dim=-1).min().item()
    ct = cos(f8.encode_text(tok), bf.encode_text(tok), dim=-1).min().item()
    dl = (f8(img, tok) - bf(img, tok)).abs().max().item()
    print(f"{name} {precision}: batch 6 (fp8 c_fc, bf16 c_proj): min cosine image {ci:.5f} text {ct:.5f}, logits max-abs diff {dl:.3f} (T = 1/0.07)")
    # e4m3 operands carry ~2^-4 relative rounding noise per element (~3 % per projection output, uncorrelated between layers).
    # Measured (deterministic), image / text, batch 6 | batch 256:
    #   fp8      ViT-B/32 0.99950 / 0.99884 | 0.99897 / 0.99693     24-layer stand-in 0.99921 / 0.99844 | 0.99814 / 0.99552
    #   fp8-qkv  ViT-B/32 0.99888 / 0.99509 | 0.99805 / 0.99225     24-layer stand-in 0.99820 / 0.99282 | 0.99695 / 0.98828
    # (in_proj's noise is amplified by the softmax of the synthetic weights' wide attention logits, most in the causal text tower)
    floors = {("fp8", "b32"): ((0.999, 0.998), (0.9985, 0.996)), ("fp8", "l16"): ((0.9985, 0.9975), (0.9975, 0.9945)),
              ("fp8-qkv", "b32"): ((0.998, 0.994), (0.995, 0.990)), ("fp8-qkv", "l16"): ((0.997, 0.99), (0.994, 0.986))}
    (fi, ft), (fib, ftb) = floors[(precision, name[:3])]
    assert ci >= fi and ct >= ft
    assert ci_b >= fib and cb >= ftb                             # ... with the e4m3 hidden matrix and fp8 c_proj on top
    assert abs(f8.contrastive_loss(img, tok).item() - bf.contrastive_loss(img, tok).item()) <= 0.1


@pytest.mark.parametrize("name,precision", [("l14-fp8-msclips", "fp8"), ("l14-fp8-msclips", "fp8-qkv"), ("b32-yfcc-msclips", "fp8")])
def test_fp8_path_against_the_recipe_emulation(gpu_device, name, precision):
    """The fp8 path has no reference semantics; what it is checked against is the STATED recipe, emulated
    independently in fp32 torch by oracle/fp8_recipe.py (quantise / dequantise with torch's own e4m3 rounding, fp32 matmul;
    everything the recipe does not name is the fp32 oracle).  BASELINE config C5 at its batch of 256: the HIP features of
    sampled pairs against the emulation run with the engine's calibrated hidden scales.  The HIP path must sit much closer to
    the emulation of its recipe than to the plain fp32 oracle (the distance to which is the recipe's own quantisation noise)."""
    from oracle import fp8_recipe as R
    arch = O.arch_l14() if name.startswith("l14") else O.arch_b32()
    sd = synth_sd(name)
    m = _model_with(name, ["MODEL.SPEC.PRECISION", precision])
    eng = m.engine()
    B = 256
    st = eng.calibrate_fp8(synth.synth_images(B, seed=35).cuda(), synth.synth_tokens(B, seed=36).cuda())
    img, tok = synth.synth_images(B, seed=37).cuda(), synth.synth_tokens(B, seed=38).cuda()
    w = eng.run(img, tok)
    fi, ft = w["fv"].clone().cpu(), w["ft"].clone().cpu()
    pre = {"v": "visual.transformer.resblocks.", "t": "transformer.resblocks."}
    scales = {pre[k.split(".")[1]] + k.split(".")[0]: v for k, v in st.items()}
    last = eng.n_layers - 1
    tail = {pre["v"] + str(last), pre["t"] + str(last)}          # the last block's MLP runs on the live rows in bf16 (no fp8)
    rec = {}
    blk = R.make_block_fn(precision, scales, record=rec, live_tail=tail)
    pick_i, pick_t = [0, B - 1], [1, B - 2]
    cos = torch.nn.functional.cosine_similarity
    with torch.no_grad():
        ei = O.encode_image(img[pick_i].cpu(), sd, arch, block_fn=blk)
        et = O.encode_text(tok[pick_t].cpu(), sd, arch, block_fn=blk)
        pi, pt = O.encode_image(img[pick_i].cpu(), sd, arch), O.encode_text(tok[pick_t].cpu(), sd, arch)
    c_emul = min(cos(fi[pick_i], ei, dim=-1).min().item(), cos(ft[pick_t], et, dim=-1).min().item())
    c_plain = min(cos(fi[pick_i], pi, dim=-1).min().item(), cos(ft[pick_t], pt, dim=-1).min().item())
    c_rec = min(cos(ei, pi, dim=-1).min().item(), cos(et, pt, dim=-1).min().item())
    print(f"{name} {precision}: min cosine HIP vs recipe emulation {c_emul:.6f}; HIP vs fp32 oracle {c_plain:.6f}; "
          f"emulation vs fp32 oracle {c_rec:.6f}")
    # End to end, e4m3 rounding decisions decorrelate between two implementations of one recipe (a last-bit difference in a
    # LayerNorm output flips a rounding, and 24 layers amplify it), so the features can only say "no further from the recipe than
    # from plain fp32"; the layer-level test below (same inputs, one block) is the tight one.
    assert c_emul >= c_plain - 2e-4 and c_emul >= (0.994 if precision == "fp8-qkv" else 0.9965)
    assert abs((1 - c_plain) - (1 - c_rec)) <= 0.6 * (1 - c_rec) + 1e-4      # the HIP path's distance from fp32 = the recipe's own noise level
    # the calibrated scales: 1.25 x max |hidden| / 448 over the calibration batch -- at least what the emulation sees on the
    # sampled pairs of another batch, within a factor of the batch-to-batch spread
    for p, amax in rec.items():
        if p in scales:
            s_emul = 1.25 * amax / 448.0
            assert 0.4 * s_emul <= scales[p] <= 4.0 * s_emul, (p, scales[p], s_emul)


@pytest.mark.parametrize("name", ["b32-yfcc-msclips", "l14-fp8-msclips"])
def test_fp8_mlp_of_one_block_against_the_recipe_emulation(gpu_device, name):
    """One block's ln_2 -> c_fc -> QuickGELU -> e4m3 hidden -> c_proj -> residual under PRECISION fp8, through the engine's own
    methods (_ln_f8, _mlp_f8: the launches of the layer loop) on a given fp32 residual matrix, against oracle/fp8_recipe.py on
    the SAME rows: per-token e4m3 LayerNorm output, per-channel e4m3 weights, static calibrated hidden scale with saturation,
    fp32 accumulation.  Same inputs, so the two agree to accumulation order plus the rare e4m3 rounding-boundary flip."""
    from oracle import fp8_recipe as R
    sd = synth_sd(name)
    m = _model_with(name, ["MODEL.SPEC.PRECISION", "fp8"])
    eng = m.engine()
    B = 256
    eng.calibrate_fp8(synth.synth_images(B, seed=35).cuda(), synth.synth_tokens(B, seed=36).cuda())
    w = eng._workspace(B, B, inference=True)
    Mv, M, D = w["Mv"], w["M"], eng.D
    i = 3
    vb, tb = eng.vblk[i], eng.tblk[i]
    assert vb["w"] is tb["w"] and vb["w"].hid_scale is not None
    g = torch.Generator().manual_seed(77)
    x0 = (torch.randn(M, D, generator=g) * 1.3 + torch.randn(M, 1, generator=g) * 0.5).cuda()
    w["X"][:M].copy_(x0)
    with torch.cuda.device(eng.dev):
        eng._ln_f8(w, [(0, Mv, vb), (Mv, M, tb)], "ln2")
        eng._mlp_f8(w, 0, M, vb["w"])
    out = w["X"][:M].clone()
    rows = torch.cat([torch.arange(0, 64), torch.arange(Mv - 32, Mv + 32), torch.arange(M - 64, M)])
    pv, pt = f"visual.transformer.resblocks.{i}", f"transformer.resblocks.{i}"
    xs = x0[rows.cuda()].cpu()
    is_v = rows < Mv
    h = torch.where(is_v[:, None], O.layer_norm(xs, sd[pv + ".ln_2.weight"], sd[pv + ".ln_2.bias"]),
                    O.layer_norm(xs, sd[pt + ".ln_2.weight"], sd[pt + ".ln_2.bias"]))
    hid = O.quick_gelu(R.linear_f8(h, sd[pv + ".mlp.c_fc.weight"], sd[pv + ".mlp.c_fc.bias"]))
    s_h = vb["w"].hid_scale
    wq, sw = R.quant_rows(sd[pv + ".mlp.c_proj.weight"])
    ref = xs + (R.e4m3(hid / s_h) @ wq.t()) * (s_h * sw.t()) + sd[pv + ".mlp.c_proj.bias"]
    upd, upd_ref = (out[rows.cuda()].cpu() - xs), (ref - xs)                     # the block's contribution to the residual stream
    err = (upd - upd_ref).abs()
    scale = upd_ref.abs().max().item()
    print(f"{name}: fp8 MLP update vs recipe emulation: max err {err.max().item():.3e}, mean {err.mean().item():.3e} (update abs-max {scale:.3f}, "
          f"saturated hidden values {(hid.abs() / s_h > 448).float().mean().item():.2e})")
    assert err.max().item() <= 2e-2 * scale and err.mean().item() <= 1.5e-3 * scale
    cosr = torch.nn.functional.cosine_similarity(upd, upd_ref, dim=-1).min().item()
    assert cosr >= 0.9998, cosr


# ---------------------------------------------------------------------------------------------------------------------
# round 4: the LayerNorm fold (engine._blocks with _fold_eligible true)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("b32-yfcc-msclips", 256), ("b16-yfcc-msclips", 256)])
def test_layernorm_fold_against_the_unfused_layer_loop(gpu_device, monkeypatch, name, B):
    """The layer loop with the LayerNorms folded into the GEMMs around them (out_proj / c_proj write the next projection's
    bf16 operand (x - centre) + row partials, in_proj / c_fc apply rstd / mean / gamma / beta on their accumulators) against the
    same engine with MSCLIP_LN_FOLD=0 (a LayerNorm pass per ln_1 / ln_2, M.py:1027-1028): every per-block tap of both towers,
    the features, image-only and text-only calls.  Both paths round the same quantities to bf16 at different points, so they
    agree to bf16-operand noise; each is separately pinned to the oracle at these sizes (test_full_bench_batch_properties,
    test_full_batch_b16_against_oracle, test_c4_per_rank_batch_1024_against_oracle run the fold)."""
    from msclip_amd import hip
    m = model_for(name)
    img = synth.synth_images(B, seed=51).cuda()
    tok = synth.synth_tokens(B, seed=52).cuda()
    eng = m.engine()
    calls = []
    real = hip.rowstat_finalize
    monkeypatch.setattr(hip, "rowstat_finalize", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    set_opt(monkeypatch, m, ln_fold=False, plan=False)            # (plan off: this test counts calls of the Python binding)
    t0 = {}
    w = eng.run(img, tok, taps=t0)
    f0i, f0t = w["fv"].clone(), w["ft"].clone()
    assert not calls
    set_opt(monkeypatch, m, ln_fold=True)
    t1 = {}
    w = eng.run(img, tok, taps=t1)
    f1i, f1t = w["fv"].clone(), w["ft"].clone()
    assert len(calls) >= 2 * (eng.n_layers - 2)                     # the fold ran: one finalize per folded LayerNorm
    blocks = [k for k in t0 if k.startswith("vblock") or k.startswith("tblock") or k.startswith("adapter")]
    assert len(blocks) >= 2 * (eng.n_layers - 1)
    worst = 0.0
    for k in blocks:
        a, b = t0[k], t1[k]
        err = (a - b).abs().max().item() / max(a.abs().max().item(), 1e-3)
        worst = max(worst, err)
        assert err <= 1.5e-2, (k, err)
        assert torch.nn.functional.cosine_similarity(a.flatten(1), b.flatten(1), dim=-1).min().item() >= 0.9999, k
    for a, b in ((f0i, f1i), (f0t, f1t)):
        assert (a - b).abs().max().item() <= 2e-3
        assert torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item() >= 0.99995
    # the shipped schedule (no taps: live-row tail of the last block, side streams), then single-tower calls
    calls.clear()
    w = eng.run(img, tok)
    assert calls and (w["fv"] - f0i).abs().max().item() <= 2e-3 and (w["ft"] - f0t).abs().max().item() <= 2e-3
    assert (m.encode_image(img) - f0i).abs().max().item() <= 2e-3
    assert (m.encode_text(tok) - f0t).abs().max().item() <= 2e-3
    for _ in range(2):                                               # repeatable bit for bit (buffer reuse across steps)
        w2 = eng.run(img, tok)
        assert torch.equal(w2["fv"], w["fv"]) and torch.equal(w2["ft"], w["ft"])
    print(f"{name}: fold vs unfused, worst tap deviation {worst:.2e} of abs-max")
    if name.startswith("b32"):
        # hipGraph replay of the folded step is bitwise the eager one
        replay = eng.graph(B, B)
        wg = replay(img, tok)
        assert torch.equal(wg["fv"], w["fv"]) and torch.equal(wg["ft"], w["ft"])
        # an in-place change of a LayerNorm's gamma / beta reaches the gamma-folded weights (re-pack on the next call)
        m2 = _model_with(name, [])
        e2 = m2.engine()
        e2.run(img, tok)                                   # the gamma-folded copies of the original weights exist now
        ln = m2.visual.transformer.resblocks[3].ln_2
        with torch.no_grad():
            ln.weight.mul_(1.5)
            ln.bias.add_(0.25)
        a = e2.run(img, tok)["fv"].clone()
        set_opt(monkeypatch, m2, ln_fold=False)
        b = e2.run(img, tok)["fv"].clone()
        set_opt(monkeypatch, m2, ln_fold=True)
        assert (a - b).abs().max().item() <= 2e-3 and (a - f0i).abs().max().item() > 5e-3      # both paths moved, together


def test_bitwise_repeatable_across_fresh_workspaces_with_side_streams(gpu_device):
    """Round 4 found (and fixed) a store-data hazard in the fused front kernel that only showed when text block 0 ran on its side
    stream beside it AND the workspace was fresh: single dwords of the stage-0 map came out wrong, ~1 run in 5, 1e-3 on the image
    features (a reused workspace hides such faults: stale values equal the right ones).  The BASELINE C2 step, twelve times, each
    into a new workspace carved from NaN-poisoned memory: bit for bit the same features, no NaN."""
    m = model_for("b32-yfcc-msclips")
    eng = m.engine()
    B = 512
    img, tok = synth.synth_images(B, seed=51).cuda(), synth.synth_tokens(B, seed=52).cuda()
    ref = None
    for rep in range(12):
        eng._ws = {k: v for k, v in eng._ws.items() if k == "loss_ws"}
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        junk = torch.full((int(6e9) // 4,), float("nan"), device="cuda")
        del junk
        w = eng.run(img, tok)
        fi, ft = w["fv"].clone(), w["ft"].clone()
        assert torch.isfinite(fi).all() and torch.isfinite(ft).all()
        if ref is None:
            ref = (fi, ft)
        assert torch.equal(fi, ref[0]) and torch.equal(ft, ref[1]), rep

# ---------------------------------------------------------------------------------------------------------------------
# round 5: the fused in_proj + attention kernel as an opt-in engine path (MSCLIP_FUSED_QKV_ATTN=1)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pack", [True, False])
def test_fused_qkv_attention_engine_path_against_reference_goldens(gpu_device, monkeypatch, pack):
    """MSCLIP_FUSED_QKV_ATTN=1 (msclip_qkv_attention in the layers whose attention tensors are shared) on the golden batch of
    the REAL reference: features, logits and the reference's block taps (blocks 1 / 2 / 11 of both towers) within the same
    tolerances as the default path, packed captions and full rows."""
    from conftest import summarize
    from msclip_amd import hip
    name = "b32-yfcc-msclips"
    g = golden(name)
    m = model_for(name)
    set_opt(monkeypatch, m, fused_qkv_attn=True, text_pack=bool(pack), plan=False)     # (plan off: the binding's calls are counted)
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    calls = []
    real = hip.qkv_attention
    monkeypatch.setattr(hip, "qkv_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    taps = {}
    w = m.engine().run(img, tok, taps=taps)
    assert len(calls) == m.engine().n_layers - 1                      # every shared layer took the fused kernel (taps: full last block)
    fi, ft = w["fv"].float().cpu().numpy(), w["ft"].float().cpu().numpy()
    assert np.abs(fi - g["image_features"]).max() <= 5e-3 and np.abs(ft - g["text_features"]).max() <= 5e-3
    for k in [k[4:] for k in g.files if k.startswith("tap_") and ("block" in k)]:
        t = taps[k]
        got, ref = summarize(t), g["tap_" + k]
        scale = max(np.abs(ref[2:]).max(), 1e-3)
        if k.startswith("tblock") and pack:
            live = _live_sample_mask(t.shape, taps["text_lengths"])
            err = np.abs(got[2:] - ref[2:])[live].max() / scale
        else:
            err = np.abs(got[2:] - ref[2:]).max() / scale
        assert err <= 4e-2, (k, err)
    calls.clear()
    logits = m(img, tok).float().cpu().numpy()                        # the shipped schedule (side streams, live-row last block)
    assert calls and np.abs(logits - g["logits"]).max() <= 0.05


def test_fused_qkv_attention_engine_path_with_the_layernorm_fold(gpu_device, monkeypatch):
    """The same opt-in path at batch 256, where the LayerNorm fold runs (per-modality gamma-folded weights, rstd / mean in the
    fused kernel's staging step): features against the default path on the same inputs, bitwise repeatable."""
    name, B = "b32-yfcc-msclips", 256
    m = model_for(name)
    img = synth.synth_images(B, seed=61).cuda()
    tok = synth.synth_tokens(B, seed=62).cuda()
    eng = m.engine()
    w = eng.run(img, tok)
    f0i, f0t = w["fv"].clone(), w["ft"].clone()
    set_opt(monkeypatch, m, fused_qkv_attn=True)
    w = eng.run(img, tok)
    f1i, f1t = w["fv"].clone(), w["ft"].clone()
    for a, b in ((f0i, f1i), (f0t, f1t)):
        assert (a - b).abs().max().item() <= 2e-3
        assert torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item() >= 0.99995
    w = eng.run(img, tok)
    assert torch.equal(w["fv"], f1i) and torch.equal(w["ft"], f1t)


def test_eval_input_pipeline_matches_the_single_threaded_loader(gpu_device, tmp_path):
    """msclip_amd.zeroshot.ImagePipeline (decoding threads -> pinned uint8 staging -> copy stream -> normalisation by table look-up
    on the GPU; reference tools/zero_shot.py:70-81, 202-217, 262) against the single-threaded PIL + numpy loop that defines the
    arithmetic: the pixel tensors are bit-identical, hence logits and top-1 too -- over several batches incl. a ragged last one,
    mixed sizes / modes (RGB, L, RGBA, portrait / landscape)."""
    from PIL import Image
    from msclip_amd import zeroshot
    rng = np.random.default_rng(11)
    n_cls, per = 4, 9
    for c in range(n_cls):
        (tmp_path / "val" / f"n{c:02d}").mkdir(parents=True)
        for k in range(per):
            h, w = int(rng.integers(180, 420)), int(rng.integers(180, 420))
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            img = Image.fromarray(a)
            if k % 4 == 1:
                img = img.convert("L")
            if k % 4 == 2:
                img = img.convert("RGBA")
            img.save(tmp_path / "val" / f"n{c:02d}" / f"{k}.{'png' if (k % 2 or img.mode == 'RGBA') else 'jpg'}")
    _, items = zeroshot.image_folder(str(tmp_path / "val"))
    pipe = zeroshot.ImagePipeline(items, 8, "cuda", workers=4)
    got = [(x.clone(), y.clone(), n) for x, y, n in pipe]
    pipe.close()
    assert sum(n for _, _, n in got) == len(items) == n_cls * per and got[-1][2] == len(items) % 8
    ref = torch.stack([zeroshot.preprocess(Image.open(p)) for p, _ in items])
    assert torch.equal(torch.cat([x for x, _, _ in got]).cpu(), ref)
    assert torch.cat([y for _, y, _ in got]).cpu().tolist() == [c for _, c in items]
    m = model_for("b32-yfcc-msclips")

    class Tok:
        def __call__(self, texts, context_length=77):
            return synth.synth_tokens(len(texts), seed=len(texts[0]))
    classes, templates = [f"c{i}" for i in range(n_cls)], ["a photo of a {}.", "art of the {}."]
    a = zeroshot.evaluate(m, Tok(), str(tmp_path / "val"), classes, templates, batch_size=8, log=lambda s: None, return_logits=True, workers=3)
    b = zeroshot.evaluate(m, Tok(), str(tmp_path / "val"), classes, templates, batch_size=8, log=lambda s: None, return_logits=True, workers=0)
    assert torch.equal(a["logits"], b["logits"]) and a["top1"] == b["top1"] and a["n"] == b["n"] == len(items)
    assert a["loader_threads"] == 3 and b["loader_threads"] == 0 and a["images_per_s"] > 0
    # decoding PROCESSES (plain subprocesses writing shared memory): the same pixels again
    c = zeroshot.evaluate(m, Tok(), str(tmp_path / "val"), classes, templates, batch_size=8, log=lambda s: None, return_logits=True, processes=3)
    assert torch.equal(c["logits"], b["logits"]) and c["loader_processes"] == 3 and c["loader_threads"] == 0
