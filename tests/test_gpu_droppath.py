"""Stochastic depth (MODEL.SPEC.VISION.DROP_PATH) on a real MI355X: the row-scaled kernels one by one, then the training step
with replayed masks against the oracle helper (tests/droppath_ref.py, pinned against the reference module in
tests/test_droppath_cpu.py), the off path, the mask generator, accumulate() and inference.

Bounds are the suite's own, unchanged: the residual GEMM's tolerance of tests/test_gpu_kernels.py::test_gemm_epilogues, the
feature / loss bounds of tests/test_gpu_model.py and tests/test_gpu_train_full.py, tests/gradcheck.py with the r of
tests/golden/train_full_gradient_ratios.json."""
import json
import os

import pytest
import torch

import droppath_ref as R
import gradcheck as G
from conftest import GOLDEN, synth_sd
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O
from oracle.autograd import parameter_aliases

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B32, L14 = "b32-yfcc-msclips", "l14-fp8-msclips"
FEAT_TOL, COS_TOL, LOSS_TOL = 5e-3, 0.9999, 2e-2          # tests/test_gpu_model.py, tests/test_gpu_train_full.py
P, KEEP = 0.25, 0.75
TOK = "token_embedding.weight"


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def close(got, ref, atol, rtol=0.0):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    assert bool((err <= atol + rtol * ref.abs()).all()), f"max err {err.max().item():.4g} (ref absmax {ref.abs().max().item():.4g})"


def bits(t):
    return t.contiguous().view(torch.int32)


def scale_pattern(M):
    """0, 1, 1 / 0.75, 1 / 0.9 so that any 4 consecutive rows -- hence every 256-row tile, every wave's 128 rows and every group of
    rows one lane owns -- hold all four, with the phase shifting every 8 and every 32 rows."""
    vals = torch.tensor([0.0, 1.0, 1.0 / 0.75, 1.0 / 0.9], dtype=torch.float32)
    m = torch.arange(M)
    return vals[(m + m // 8 + m // 32) % 4].cuda()


# ---------------------------------------------------------------------------- 1. the GEMM epilogue
@pytest.mark.parametrize("M,N,K,tile,variant", [(512, 768, 768, 4, "pp"), (200, 64, 64, 0, "dense128"), (37, 66, 64, 0, "dense128")],
                         ids=["pingpong", "generic-vectorised", "generic-tail"])
def test_gemm_row_scale(gpu_device, M, N, K, tile, variant):
    x, w, b = rnd(M, K, seed=1, dtype=BF), rnd(N, K, seed=2, scale=0.05, dtype=BF), rnd(N, seed=3)
    resid = rnd(M, N, seed=4)
    resid[0, 0], resid[4, 1] = -0.0, 1e-41                                   # a signed zero and a denormal must come through a dropped row (0, 4)
    s = scale_pattern(M)
    assert hip.gemm_variant(hip.describe_gemm(0, M, N, K, tile=tile, resid_kind=hip.RESID_F32)) == variant
    plain = torch.full((M + 2, N), float("nan"), device="cuda")
    hip.gemm(x, w, plain[:M], bias=b, resid=resid, resid_kind=hip.RESID_F32, tile=tile)
    out = torch.full((M + 2, N), float("nan"), device="cuda")
    for _ in range(2):
        hip.gemm(x, w, out[:M], bias=b, resid=resid, resid_kind=hip.RESID_F32, tile=tile, row_scale=s)
    assert bool(torch.isnan(out[M:]).all())                                  # nothing written past M
    one, zero = s == 1.0, s == 0.0
    assert int(one.sum()) >= M // 5 and int(zero.sum()) >= M // 5
    assert torch.equal(bits(out[:M][one]), bits(plain[:M][one]))             # scale 1.0f: bitwise the launch without a scale
    assert torch.equal(bits(out[:M][zero]), bits(resid[zero]))               # scale 0.0f: bitwise the residual
    ref = resid + s[:, None] * (x.float() @ w.float().t() + b)
    close(out[:M], ref, 2e-3, 1e-4)                                          # test_gemm_epilogues' bound for the fp32 residual update
    # in place (resid == out), as the inference path runs its residual updates
    inpl = resid.clone()
    hip.gemm(x, w, inpl, bias=b, resid=inpl, resid_kind=hip.RESID_F32, tile=tile, row_scale=s)
    assert torch.equal(bits(inpl), bits(out[:M]))
    # a branch value that is not finite does not leak into a dropped row
    xbad = x.clone()
    xbad[zero.nonzero()[0], 3] = float("inf")
    hip.gemm(xbad, w, inpl.copy_(resid), bias=b, resid=resid, resid_kind=hip.RESID_F32, tile=tile, row_scale=s)
    assert torch.equal(bits(inpl[zero]), bits(resid[zero]))


def test_gemm_row_scale_with_a_device_row_count(gpu_device):
    """M_dev (packed captions): the ping-pong kernel runs min(M, *M_dev) rows -- a ragged last tile goes through its guarded
    epilogue -- and the table is indexed by the launch's row."""
    M, N, K, live = 768, 768, 768, 300
    x, w, b = rnd(M, K, seed=1, dtype=BF), rnd(N, K, seed=2, scale=0.05, dtype=BF), rnd(N, seed=3)
    resid, s = rnd(M, N, seed=4), scale_pattern(M)
    full = torch.empty(M, N, device="cuda")
    hip.gemm(x, w, full, bias=b, resid=resid, resid_kind=hip.RESID_F32, tile=4, row_scale=s)
    out = torch.full((M, N), float("nan"), device="cuda")
    mdev = torch.tensor([live], dtype=torch.int32, device="cuda")
    hip.gemm(x, w, out, bias=b, resid=resid, resid_kind=hip.RESID_F32, row_scale=s, mdev=mdev)
    assert bool(torch.isnan(out[live:]).all())
    assert torch.equal(bits(out[:256]), bits(full[:256]))                    # the whole tile: the same epilogue
    zero = (s == 0.0)[:live]
    assert torch.equal(bits(out[:live][zero]), bits(resid[:live][zero]))
    close(out[:live], resid[:live] + s[:live, None] * (x[:live].float() @ w.float().t() + b), 2e-3, 1e-4)
    plain = torch.empty(M, N, device="cuda")
    hip.gemm(x, w, plain, bias=b, resid=resid, resid_kind=hip.RESID_F32, mdev=mdev)
    one = (s == 1.0)[:live]
    assert torch.equal(bits(out[:live][one]), bits(plain[:live][one]))


def test_gemm_row_scale_is_refused_where_it_is_not_implemented(gpu_device):
    M, D, K = 512, 768, 768
    a, w, b = rnd(M, K, seed=71, dtype=BF), rnd(D, K, seed=72, scale=0.03, dtype=BF), rnd(D, seed=73)
    x0, s = rnd(M, D, seed=74), scale_pattern(M)
    fo = hip.FoldOut(torch.empty(M, D, dtype=BF, device="cuda"), x0.mean(dim=1), torch.empty(M, D // 64, 2, device="cuda"))
    out = x0.clone()
    with pytest.raises(hip.HipError, match="msclip_gemm_rowscale.*-1"):       # the LayerNorm fold's producer form
        hip.gemm(a, w, out, bias=b, resid=out, resid_kind=hip.RESID_F32, fold_out=fo, row_scale=s)
    assert torch.equal(out, x0)                                              # nothing ran
    o16 = torch.empty(M, D, dtype=BF, device="cuda")
    r16 = x0.to(BF)
    for kw in (dict(out=o16), dict(out=o16, resid=r16, resid_kind=hip.RESID_BF16), dict(out=out, resid=r16, resid_kind=hip.RESID_BF16),
               dict(out=out, resid=out, resid_kind=hip.RESID_F32, act=hip.ACT_QUICKGELU), dict(out=out),
               dict(out=o16, out2=torch.empty_like(o16), act=hip.ACT_QUICKGELU)):
        o = kw.pop("out")
        with pytest.raises(hip.HipError, match="-1"):
            hip.gemm(a, w, o, bias=b, row_scale=s, **kw)
    hip.gemm(a, w, out, bias=b, resid=out, resid_kind=hip.RESID_F32, fold_out=fo)           # the same launch without a scale is fine


# ---------------------------------------------------------------------------- 2. LayerNorm backward, cast + column sums
@pytest.mark.parametrize("dy_f32", [True, False])
def test_layernorm_backward_row_scale(gpu_device, dy_f32):
    M, C = 300, 768
    x, gam = rnd(M, C, seed=1) + 0.3, rnd(C, seed=2) * 0.2 + 1.0
    dy = rnd(M, C, seed=3, dtype=torch.float32 if dy_f32 else BF)
    dx0, s = rnd(M, C, seed=4), scale_pattern(M)

    def run(scale):
        dx, dxb = dx0.clone(), torch.full((M, C), float("nan"), dtype=BF, device="cuda")
        part = torch.full((hip.LN_PART_BLOCKS, C), float("nan"), device="cuda")
        pg, _ = hip.layernorm_bwd(x, dy, gam, dx, M, dxb=dxb, sum_part=part, fold=False, row_scale=scale)
        return dx, dxb, hip.colsum(part), pg
    dx_p, dxb_p, sum_p, pg_p = run(None)
    dx_s, dxb_s, sum_s, pg_s = run(s)
    assert torch.equal(bits(dx_s), bits(dx_p))                               # dX itself is untouched by the scale
    assert torch.equal(bits(pg_s), bits(pg_p))                               # so are the LayerNorm's own parameter gradients
    assert torch.equal(dxb_s.view(torch.int16), (s[:, None] * dx_p).to(BF).view(torch.int16))
    assert torch.equal(dxb_s[s == 1.0].view(torch.int16), dxb_p[s == 1.0].view(torch.int16))
    ref = (s[:, None].double() * dx_p.double()).sum(0)
    bound = 2e-6 * (s[:, None] * dx_p).abs().double().sum(0).max().item()    # tests/test_gpu_train.py::test_layernorm_backward's bound
    assert (sum_s.double() - ref).abs().max().item() <= bound
    assert (sum_p.double() - dx_p.double().sum(0)).abs().max().item() <= bound
    # an all-ones table: bitwise the entry point without a scale
    dx_1, dxb_1, sum_1, _ = run(torch.ones(M, device="cuda"))
    assert torch.equal(bits(dx_1), bits(dx_p)) and torch.equal(dxb_1.view(torch.int16), dxb_p.view(torch.int16))
    assert torch.equal(bits(sum_1), bits(sum_p))


def test_cast_with_column_sums_row_scale(gpu_device):
    M, C = 300, 768
    buf = rnd(M + 3, C + 8, seed=5)
    x, s = buf[:M, :C], scale_pattern(M)
    keep = buf.clone()
    y, sums = hip.cast_bf16_colsum(x, row_scale=s)
    assert torch.equal(bits(buf), bits(keep))                                # the input is only read
    assert torch.equal(y.view(torch.int16), (s[:, None] * x).to(BF).view(torch.int16))
    ref = (s[:, None].double() * x.double()).sum(0)
    assert (sums.double() - ref).abs().max().item() <= 2e-6 * (s[:, None] * x).abs().double().sum(0).max().item()
    y1, sums1 = hip.cast_bf16_colsum(x, row_scale=torch.ones(M, device="cuda"))
    y0, sums0 = hip.cast_bf16_colsum(x)
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)) and torch.equal(bits(sums1), bits(sums0))
    # the compact last block's shape: a handful of rows
    yc, sc = hip.cast_bf16_colsum(x[:8], row_scale=s[:8])
    assert torch.equal(yc.view(torch.int16), (s[:8, None] * x[:8]).to(BF).view(torch.int16))
    assert (sc.double() - (s[:8, None].double() * x[:8].double()).sum(0)).abs().max().item() <= 1e-5


# ---------------------------------------------------------------------------- the model
def build(name, *opts):
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16", *opts]))
    m.load_state_dict(synth_sd(name), strict=True)
    return m.cuda().eval(), parameter_aliases(m)


def check_feats(got, ref):
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs().max().item()
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1).min().item()
    assert err <= FEAT_TOL and cos >= COS_TOL, f"max-abs {err:.3e}, min cos {cos:.6f}"
    return err, cos


def load_r():
    with open(os.path.join(GOLDEN, "train_full_gradient_ratios.json")) as f:
        d = json.load(f)
    assert 0 < d["r"] <= G.R_MAX and abs(d["r"] - min(G.R_MAX, 1.25 * d["measured_worst_ratio"])) < 1e-9
    return d["r"]


# ---------------------------------------------------------------------------- 3. forward
@pytest.mark.parametrize("mode,bn", [("sample", "frozen"), ("sample", "batch"), ("position", "frozen")])
def test_training_forward_with_replayed_masks(gpu_device, mode, bn):
    """ViT-B/32, 4 pairs.  Every vision block (the lateral-adapter layers 2, 4, .. and the compact last block included) drops at
    least one draw and keeps at least one in both branches.  Bounds: the loss bound of the training tests (2e-2) in both
    BatchNorm modes.  Features: the suite's feature bounds against the oracle (tests/test_gpu_model.py: 5e-3 / cosine 0.9999)
    were set with frozen statistics -- no existing test bounds train-mode features -- and hold here for "frozen"; with batch
    statistics of 4 images the bf16 conv maps enter every normalisation, so the yardstick is the helper's own bf16-autocast
    run, with tests/gradcheck.py's factor and margins (1.25 x its error + 5e-3, its cosine - 5e-3), never anything the
    step itself produces.  First GPU run (sample, batch): max-abs 4.7e-3, cosine 0.99956 against the fp32 helper."""
    m, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", str(P))
    arch = O.arch_b32()
    img, tok = synth.synth_images(4, seed=0), synth.synth_tokens(4, seed=1)
    masks = R.mixed_masks(arch, 4, mode)
    ts = train.TrainStep(m, lr=1e-4, bn=bn, drop_path_mode=mode)
    assert ts.drop_path == P and ts.drop_mask_shape(4) == tuple(masks.shape)
    loss = ts.forward(img.cuda(), tok.cuda(), drop_masks=masks).item()
    assert torch.equal(ts.last_drop_masks.cpu(), masks)
    assert ts.saved["layers"][-1].get("compact") is not None and ts.saved["layers"][2]["adapter"] is not None
    fv, ft = ts.saved["fv"].clone(), ts.saved["ft"].clone()
    ri, rt, ref_loss = R.droppath_forward(synth_sd(B32), arch, img, tok, masks, mode, KEEP, bn_train=bn == "batch")
    if bn == "batch":
        yi, _, _ = R.droppath_forward(synth_sd(B32), arch, img, tok, masks, mode, KEEP, bn_train=True, autocast_bf16=True)
        yerr = (yi - ri).abs().max().item()
        ycos = torch.nn.functional.cosine_similarity(yi, ri, dim=-1).min().item()
        got = fv.float().cpu()
        ei, ci = (got - ri).abs().max().item(), torch.nn.functional.cosine_similarity(got, ri, dim=-1).min().item()
        print(f"train-mode BatchNorm image features: max-abs {ei:.3e} (bf16 helper {yerr:.3e}), min cosine {ci:.6f} ({ycos:.6f})")
        assert ei <= G.MEDIAN_FACTOR * yerr + G.MEDIAN_MARGIN and ci >= ycos - G.COS_MARGIN, (ei, yerr, ci, ycos)
    else:
        ei, ci = check_feats(fv, ri)
    et, ct = check_feats(ft, rt)
    with torch.no_grad():
        plain = O.encode_image(img, synth_sd(B32), arch)
    moved = (plain - ri).abs().max().item()
    print(f"{mode} {bn}: loss {loss:.5f} (helper {ref_loss:.5f}); image max-abs {ei:.2e} cos {ci:.6f}; text {et:.2e} {ct:.6f}; "
          f"the masks moved the image features by {moved:.3f}")
    assert abs(loss - ref_loss) <= LOSS_TOL
    assert moved > 10 * FEAT_TOL                                             # a forward that ignored the masks would not pass
    with pytest.raises(ValueError, match="drop_masks"):
        ts.forward(img.cuda(), tok.cuda(), drop_masks=masks[:, :, :1])


# ---------------------------------------------------------------------------- 4. gradients (and 8. accumulate: the same reference)
_REF = {}


def reference(mode, bn):
    """(img, tok, masks, measure(yardstick), fp32 helper gradients, helper loss) for ViT-B/32 at batch 8, computed once."""
    if (mode, bn) not in _REF:
        arch = O.arch_b32()
        img, tok = synth.synth_images(8, seed=0), synth.synth_tokens(8, seed=1)
        masks = R.mixed_masks(arch, 8, mode, seed=2)
        m = get_clip_model(named_config(B32))
        alias = parameter_aliases(m)
        kw = dict(aliases=alias, bn_train=bn == "batch")
        ref, ref_loss = R.droppath_gradients(synth_sd(B32), arch, img, tok, masks, mode, KEEP, **kw)
        yard, _ = R.droppath_gradients(synth_sd(B32), arch, img, tok, masks, mode, KEEP, autocast_bf16=True, **kw)
        assert len(ref) == 325
        _REF[(mode, bn)] = (img, tok, masks, G.measure(yard, ref), ref, ref_loss)
    return _REF[(mode, bn)]


@pytest.mark.parametrize("mode,bn", [("sample", "frozen"), ("position", "batch")])
def test_every_gradient_element_against_the_helper_autograd(gpu_device, mode, bn):
    """tests/gradcheck.py's comparison with test_gpu_train_full.py's bounds.  A backward without the scale in the dgrad operand,
    the weight gradient or the bias sums of out_proj / c_proj differs from this reference in those tensors (and in everything
    upstream) by the size of the dropped share; tests/test_droppath_cpu.py shows the bounds report the bias sums' case."""
    img, tok, masks, ym, ref, ref_loss = reference(mode, bn)
    m, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", str(P))
    ts = train.TrainStep(m, lr=1e-4, bn=bn, drop_path_mode=mode)
    loss = ts.forward(img.cuda(), tok.cuda(), drop_masks=masks).item()
    grads = {k: g.detach().float().cpu() for k, g in ts.backward().items()}
    got = G.measure(grads, ref)
    print(f"{mode} {bn}: loss {loss:.5f} (helper {ref_loss:.5f})")
    print(G.describe(f"b32-{mode}-{bn}-b8", got, ym))
    assert abs(loss - ref_loss) <= LOSS_TOL
    bad = G.violations(got, ym, load_r())
    assert not bad, "\n".join(bad)


def test_accumulate_with_replayed_masks_is_the_one_shot_step(gpu_device):
    """2 chunks of 4 with per-chunk masks, frozen BatchNorm, against ONE step on the 8 pairs with the concatenated masks: the
    bound tests/test_gpu_accumulate.py puts on chunked against one-shot -- tests/gradcheck.py against the one-shot reference,
    the same r -- plus the GPU one-shot step itself held to it; both feature passes of a chunk used the same masks
    (check_features)."""
    img, tok, masks, ym, ref, ref_loss = reference("sample", "frozen")
    m, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", str(P))
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    chunks = [(img[:4].cuda(), tok[:4].cuda()), (img[4:].cuda(), tok[4:].cuda())]
    per_chunk = [masks[:, :, :4].contiguous(), masks[:, :, 4:].contiguous()]
    loss, grads = ts.accumulate(chunks, drop_masks=per_chunk, check_features=True)
    assert [tuple(t.shape) for t in ts.last_drop_masks] == [(11, 2, 4), (11, 2, 4)]
    got = G.measure({k: g.detach().float().cpu() for k, g in grads.items()}, ref)
    print(f"accumulate 4+4: loss {loss.item():.5f} (helper one-shot {ref_loss:.5f})")
    print(G.describe("b32-sample-frozen-4+4", got, ym))
    assert abs(loss.item() - ref_loss) <= LOSS_TOL
    bad = G.violations(got, ym, load_r())
    assert not bad, "\n".join(bad)
    with pytest.raises(ValueError, match="drop_masks"):
        ts.accumulate(chunks, drop_masks=per_chunk[:1])
    # drawn masks: one set per chunk, the same in both passes (check_features compares the banked and the recomputed features)
    ts.accumulate(chunks, check_features=True)
    a, b = ts.last_drop_masks
    assert a.shape == b.shape == (11, 2, 4) and a.dtype == torch.bool and not torch.equal(a, b)


# ---------------------------------------------------------------------------- 5. ViT-L/14
def test_l14_patch_conv_forward_with_replayed_masks(gpu_device):
    """257 tokens, 24 vision blocks from slot 0, no adapters; batch 2, forward only."""
    m, _ = build(L14, "MODEL.SPEC.VISION.DROP_PATH", str(P))
    arch = O.arch_l14()
    img, tok = synth.synth_images(2, size=arch.image_size, seed=0), synth.synth_tokens(2, seed=1)
    masks = R.mixed_masks(arch, 2, "sample")
    assert masks.shape == (24, 2, 2)
    ts = train.TrainStep(m, lr=1e-4)
    loss = ts.forward(img.cuda(), tok.cuda(), drop_masks=masks).item()
    fv, ft = ts.saved["fv"].clone(), ts.saved["ft"].clone()
    ts._release_saved()
    ri, rt, ref_loss = R.droppath_forward(synth_sd(L14), arch, img, tok, masks, "sample", KEEP)
    ei, ci = check_feats(fv, ri)
    et, ct = check_feats(ft, rt)
    print(f"l14: loss {loss:.5f} (helper {ref_loss:.5f}); image max-abs {ei:.2e} cos {ci:.6f}; text {et:.2e} {ct:.6f}")
    assert abs(loss - ref_loss) <= LOSS_TOL


# ---------------------------------------------------------------------------- 6. the off path
def test_off_path_is_bitwise_the_step_without_the_option(gpu_device):
    img, tok = synth.synth_images(8, seed=0).cuda(), synth.synth_tokens(8, seed=1).cuda()

    def step(**kw):
        masks = kw.pop("masks", None)
        m, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", "0.0")
        ts = train.TrainStep(m, lr=1e-4, bn="batch", **kw)
        assert ts.drop_path == 0.0 and ts._dp_gen is None
        loss = ts.forward(img, tok, drop_masks=masks)
        assert (ts.last_drop_masks is None) == (masks is None)
        tabled = [L["rs"] is not None for L in ts.saved["layers"]]
        return loss.clone(), {k: g.clone() for k, g in ts.backward().items()}, tabled
    l0, g0, t0 = step(drop_path=None)
    l1, g1, t1 = step(drop_path=0.0)
    assert not any(t0) and not any(t1)                                       # no table was built, no launch carried a scale
    assert torch.equal(bits(l0), bits(l1)) and sorted(g0) == sorted(g1) and len(g0) == 325
    # token_embedding.weight is an atomic scatter-add (tests/test_gpu_accumulate.py): every other tensor bit for bit
    assert not [k for k in g0 if k != TOK and not torch.equal(bits(g0[k]), bits(g1[k]))]
    # all-keep masks with p = 0: the tables are active, every scale is exactly 1.0 -> the same bits
    l2, g2, t2 = step(drop_path=0.0, masks=torch.ones(11, 2, 8, dtype=torch.bool))
    assert t2 == [False] + [True] * 11
    assert torch.equal(bits(l0), bits(l2))
    differ = [k for k in g0 if k != TOK and not torch.equal(bits(g0[k]), bits(g2[k]))]
    assert not differ, differ[:8]
    t = G.measure_one(TOK, g2[TOK], g0[TOK])
    assert t["stray_rows"] == 0 and t["row_err"] <= G.WORST_MARGIN


# ---------------------------------------------------------------------------- 7. the mask generator
def test_masks_are_reproducible_and_survive_a_checkpoint(gpu_device, tmp_path):
    data = [(synth.synth_images(4, seed=20 + i).cuda(), synth.synth_tokens(4, seed=120 + i).cuda()) for i in range(4)]
    cfg = named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", "0.2"])
    assert train.drop_path_setting(cfg) == 0.2

    def fresh(**kw):
        m, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", "0.2")
        return m, train.TrainStep(m, lr=1e-4, bn="batch", **kw)

    def draws(ts, steps, optimize=False):
        out = []
        for i in steps:
            ts.forward(*data[i])
            out.append(ts.last_drop_masks.clone())
            if optimize:
                ts.step(ts.backward())
            else:
                ts._release_saved()
        return out
    ma, ta = fresh(drop_path_seed=5)
    assert ta.drop_path == 0.2 and ta.drop_path_mode == "sample"             # None took the model's rate
    a = draws(ta, range(3))
    _, tb = fresh(drop_path_seed=5)
    b = draws(tb, range(3))
    _, tc = fresh(drop_path_seed=6)
    c = draws(tc, range(3))
    assert all(x.shape == (11, 2, 4) and x.dtype == torch.bool and x.is_cuda for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))
    assert not torch.equal(a[0], a[1])                                       # the generator moves on between the forwards
    frac = torch.stack(a + c).float().mean().item()
    assert 0.65 < frac < 0.95, frac                                          # 528 draws at keep = 0.8 (sd 0.017)
    # from_config passes the config's rate through
    tf = train.from_config(ma, cfg)
    assert tf.drop_path == 0.2 and tf.drop_path_mode == "sample"
    assert train.from_config(ma, named_config(B32)).drop_path == 0.0
    # checkpoint: two optimizer steps, save, the third forward in the running process and in a resumed one
    md, td = fresh(drop_path_seed=9)
    draws(td, range(2), optimize=True)
    path = tmp_path / "checkpoint.pth"
    train.save_checkpoint(md, td, path, step=1, model_name=B32)
    obj = torch.load(path, weights_only=False)
    assert set(obj) == {"step", "model", "state_dict", "perf", "optimizer", "drop_path_rng_state"}
    want = draws(td, [2])[0]
    me, te = fresh(drop_path_seed=1234)
    assert train.resume_checkpoint(me, te, path) == 2
    assert torch.equal(draws(te, [2])[0], want)
    # a checkpoint from before the key existed: the masks restart from the seed
    del obj["drop_path_rng_state"]
    torch.save(obj, path)
    mf, tf2 = fresh(drop_path_seed=5)
    draws(tf2, [0])
    train.resume_checkpoint(mf, tf2, path)
    assert torch.equal(draws(tf2, [0])[0], a[0])


# ---------------------------------------------------------------------------- 9. inference
def test_inference_ignores_drop_path(gpu_device):
    m0, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", "0.0")
    m1, _ = build(B32, "MODEL.SPEC.VISION.DROP_PATH", "0.2")
    assert m1.drop_path == 0.2 and list(m0.state_dict()) == list(m1.state_dict())
    img, tok = synth.synth_images(4, seed=3).cuda(), synth.synth_tokens(4, seed=4).cuda()
    assert torch.equal(bits(m0.encode_image(img)), bits(m1.encode_image(img)))
    assert torch.equal(bits(m0(img, tok)), bits(m1(img, tok)))
    assert torch.equal(bits(m0.contrastive_loss(img, tok)), bits(m1.contrastive_loss(img, tok)))
