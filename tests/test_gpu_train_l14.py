"""TrainStep on BASELINE config C5 proper (experiments/model/l14-fp8-msclips.yaml, run in bf16): ViT-L/14 with the plain
patch convolution, 16 x 16 grid = 257 image tokens, width 1024, 16 heads, 24 + 24 blocks shared from block 1.

* the 209-272-token form of msclip_attention_bwd (query-blocked, K^T read transposed out of the row-major K) against fp32
  autograd, as test_gpu_train.py::test_attention_backward checks the shorter forms;
* msclip_layernorm_bwd at C = 1024 in every mode the step uses;
* the patch-conv weight gradient against autograd of F.conv2d;
* the whole step against autograd of the REAL reference (tests/golden/l14-fp8-msclips.grads.npz, tools/make_golden.py
  --grads-l14), with the token-side bounds of test_gradients_against_reference_autograd and the reference's own bf16
  deviation on this model as the yardstick (tests/golden/ref_bf16_gradient_deviation_l14.json);
* bn = "batch" / "frozen" agree bit for bit (the model has no BatchNorm), AdamW steps lower the loss, odd batches run, a
  checkpoint round trip continues the run, fp8 is refused."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import summarize, synth_sd, GOLDEN
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAME = "l14-fp8-msclips"
BF16 = ["MODEL.SPEC.PRECISION", "bf16"]
SAMPLE_TOL, ABSMEAN_TOL, COS_TOL = 0.08, 0.05, 0.995                 # test_gpu_train.py's token-side bounds
LNB_SAMPLE_TOL, LNB_ABSMEAN_TOL, LNB_COS_TOL = 0.25, 0.15, 0.95
LNB = ("ln_1.bias", "ln_2.bias", "ln_final.bias", "ln_post.bias", "ln_pre.bias")


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def rel(got, ref):
    return ((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-12)).item()


def _model(precision="bf16"):
    m = get_clip_model(named_config(NAME, ["MODEL.SPEC.PRECISION", precision]))
    m.load_state_dict(synth_sd(NAME), strict=True)
    return m.cuda().eval()


def _attention_case(ns, L, H, causal, seed):
    qkv = rnd(ns * L, 3 * H * 64, seed=seed, scale=0.7, dtype=BF)
    dout = rnd(ns * L, H * 64, seed=seed + 1, dtype=BF)
    o = torch.empty(ns * L, H * 64, dtype=BF, device="cuda")
    hip.attention(qkv, o, ns, L, H, causal)
    qf = qkv.float().requires_grad_(True)
    q, k, v = (t.reshape(ns, L, H, 64).transpose(1, 2) for t in qf.chunk(3, dim=-1))
    sc = q @ k.transpose(-1, -2)                                              # q is pre-scaled in the packed layout
    if causal:
        sc = sc + torch.full((L, L), float("-inf"), device="cuda").triu_(1)
    ref_o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(ns * L, H * 64)
    ref_o.backward(dout.float())
    dqkv = torch.full_like(qkv, float("nan"))
    hip.attention_bwd(qkv, o, dout, dqkv, ns, L, H, causal)
    assert bool(torch.isfinite(dqkv.float()).all())                          # every element written
    r = rel(dqkv, qf.grad)
    cos = F.cosine_similarity(dqkv.float().flatten(), qf.grad.flatten(), dim=0).item()
    print(f"L {L} causal {causal} samples {ns} heads {H}: rel {r:.3e} cosine {cos:.6f}")
    assert r < 3e-2
    assert cos > 0.999, cos
    return qkv, o, dout, dqkv


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", [209, 224, 240, 257, 272])
def test_attention_backward_257_token_form(gpu_device, L, causal):
    qkv, o, dout, dqkv = _attention_case(3, L, 16, causal, seed=31)
    with pytest.raises(hip.HipError):                                         # colsum_part stays refused above 96 tokens
        hip.attention_bwd(qkv, o, dout, dqkv, 3, L, 16, causal, colsum_part=torch.empty(3, 3 * 16 * 64, device="cuda"))


def test_attention_backward_257_tokens_many_pairs(gpu_device):
    """64 samples x 16 heads = 1024 (sample, head) workgroups: several per CU."""
    _attention_case(64, 257, 16, False, seed=41)


def test_attention_backward_refuses_past_its_range(gpu_device):
    L = hip.ATTENTION_BWD_MAX_L + 1
    qkv = torch.zeros(2 * L, 3 * 16 * 64, dtype=BF, device="cuda")
    o = torch.zeros(2 * L, 16 * 64, dtype=BF, device="cuda")
    with pytest.raises(hip.HipError):
        hip.attention_bwd(qkv, o, o.clone(), torch.empty_like(qkv), 2, L, 16, False)


@pytest.mark.parametrize("dy_f32,gather", [(False, False), (True, False), (False, True), (True, True)])
def test_layernorm_backward_width_1024(gpu_device, dy_f32, gather):
    """The C = 768 cases of test_gpu_train.py::test_layernorm_backward at the ViT-L width, same bounds."""
    C, M = 1024, 1000
    x = rnd(M * (3 if gather else 1), C, seed=5, scale=2.0) + 0.3
    gam, bet = rnd(C, seed=6) + 1.0, rnd(C, seed=7)
    dy = rnd(M, C, seed=8, dtype=torch.float32 if dy_f32 else BF)
    idx = (torch.arange(M, device="cuda") * 3 + 1).int() if gather else None
    xr = x[idx.long()] if gather else x
    xa = xr.clone().requires_grad_(True)
    ga, ba = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    u = xa.mean(-1, keepdim=True)
    s = (xa - u).pow(2).mean(-1, keepdim=True)
    (ga * ((xa - u) / torch.sqrt(s + 1e-12)) + ba).backward(dy.float())
    dx = torch.full_like(x, 0.5)
    dg, db = hip.layernorm_bwd(x, dy, gam, dx, M, row_idx=idx, accumulate=True)
    got = dx[idx.long()] if gather else dx
    assert rel(got - 0.5, xa.grad) < 2e-4
    if gather:
        mask = torch.ones(x.shape[0], dtype=torch.bool, device="cuda")
        mask[idx.long()] = False
        assert bool((dx[mask] == 0.5).all())                                  # untouched rows
    assert rel(dg, ga.grad) < 2e-4 and rel(db, ba.grad) < 2e-4
    dx2 = torch.full_like(x, 7.0)
    hip.layernorm_bwd(x, dy, gam, dx2, M, row_idx=idx, accumulate=False, want_param_grads=False)
    assert rel(dx2[idx.long()] if gather else dx2, xa.grad) < 2e-4
    if not gather:
        # the bf16 copy of the written rows + their per-block column sums, two row segments into one set of partials
        dx3 = torch.full_like(x, 0.5)
        dxb = torch.full((M + 3, C), 7.0, dtype=BF, device="cuda")
        part = torch.full((hip.LN_PART_BLOCKS, C), float("nan"), dtype=torch.float32, device="cuda")
        cut = 336
        dg1, db1 = hip.layernorm_bwd(x[:cut], dy[:cut], gam, dx3[:cut], cut, dxb=dxb[:cut], sum_part=part)
        dg2, db2 = hip.layernorm_bwd(x[cut:], dy[cut:], gam, dx3[cut:], M - cut, dxb=dxb[cut:M], sum_part=part, sum_accumulate=True)
        assert torch.equal(dx3, dx) and bool((dxb[M:] == 7.0).all())
        assert torch.equal(dxb[:M], hip.cast_bf16(dx)) and bool(torch.isfinite(part).all())
        assert rel(dg1 + dg2, ga.grad) < 2e-4 and rel(db1 + db2, ba.grad) < 2e-4
        ref = dx.double().sum(0)
        assert (hip.colsum(part).double() - ref).abs().max().item() <= 2e-6 * dx.abs().double().sum(0).max().item()


def test_patch_weight_gradient_against_conv_autograd(gpu_device):
    """visual.conv1.weight's gradient (TrainStep._patch_wgrad: split-K weight-gradient GEMM over msclip_patchify's matrix) for
    a given token gradient, against autograd of F.conv2d(bf16 image, W, stride=14) fed the same (bf16-rounded) grid rows."""
    m = _model()
    ts = train.TrainStep(m, lr=1e-4)
    e = ts.eng
    B, D, P, g = 3, e.D, e.S // e.g, e.g
    img = synth.synth_images(B, seed=3).cuda()
    patch = torch.zeros(B * g * g, e.patch_k, dtype=BF, device="cuda")
    hip.patchify(img, patch, B, e.S, P, e.patch_k)
    dtok = rnd(B * e.Lv, D, seed=4)
    grads = {}
    ts._patch_wgrad(grads, dtok, patch, B)
    torch.cuda.synchronize()
    from msclip_amd import gradgemm
    gradgemm.join(e.dev)
    got = grads["visual.conv1.weight"]
    assert tuple(got.shape) == (D, 3, P, P) and got.is_contiguous()
    W = m.visual.conv1.weight.detach().float().clone().requires_grad_(True)
    y = F.conv2d(img.to(BF).float(), W, stride=P)                            # [B, D, g, g]
    dgrid = dtok.view(B, e.Lv, D)[:, 1:].to(BF).float()                      # grid rows (class row excluded), as the step casts them
    y.backward(dgrid.transpose(1, 2).reshape(B, D, g, g))
    r = rel(got, W.grad)
    cos = F.cosine_similarity(got.flatten(), W.grad.flatten(), dim=0).item()
    print(f"patch weight gradient: rel {r:.3e} cosine {cos:.7f}")
    assert r < 1e-3 and cos > 0.99999


def _reference_bf16_deviation():
    with open(os.path.join(GOLDEN, "ref_bf16_gradient_deviation_l14.json")) as f:
        return json.load(f)["eval_bn_batch4"]


def test_gradients_against_reference_autograd_l14(gpu_device):
    """Every parameter's gradient against autograd of the imported reference on the golden batch (fp32 CPU, eval mode)."""
    g = np.load(os.path.join(GOLDEN, NAME + ".grads.npz"))
    m = _model()
    ts = train.TrainStep(m, lr=1e-4)
    b = int(g["batch"])
    img = synth.synth_images(b, seed=int(g["seed"])).cuda()
    tok = synth.synth_tokens(b, seed=int(g["seed"]) + 1).cuda()
    loss = ts.forward(img, tok)
    assert abs(loss.item() - float(g["loss"])) <= 2e-2, (loss.item(), float(g["loss"]))
    grads = ts.backward()
    expect = [k[2:] for k in g.files if k.startswith("g_")]
    assert len(expect) == 406
    assert sorted(grads) == sorted(expect), (sorted(set(expect) - set(grads))[:5], sorted(set(grads) - set(expect))[:5])
    worst, am, coss = {}, {}, {}
    for k in expect:
        got = grads[k]
        ref = g["g_" + k]
        sm = summarize(got)
        scale = max(float(g["gmax_" + k]), 1e-12)
        worst[k] = float(np.abs(sm[2:] - ref[2:]).max() / scale)
        am[k] = abs(sm[1] - ref[1]) / (ref[1] + 1e-12)
        if "gfull_" + k in g.files:
            full = torch.from_numpy(g["gfull_" + k]).flatten()
            coss[k] = F.cosine_similarity(got.float().cpu().flatten(), full, dim=0).item()
    print("worst sample errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])
    print("worst abs-mean deviations", sorted(am.items(), key=lambda kv: -kv[1])[:4], "lowest cosines",
          sorted(coss.items(), key=lambda kv: kv[1])[:4])
    print("visual.conv1.weight: sample error", worst["visual.conv1.weight"], "abs-mean deviation", am["visual.conv1.weight"])
    lnb_keys = [k for k in expect if k.endswith(LNB)]
    for k in expect:
        tol = (LNB_SAMPLE_TOL, LNB_ABSMEAN_TOL, LNB_COS_TOL) if k in lnb_keys else (SAMPLE_TOL, ABSMEAN_TOL, COS_TOL)
        assert worst[k] <= tol[0], (k, worst[k])
        assert am[k] <= tol[1], (k, am[k])
        if k in coss:
            assert coss[k] >= tol[2], (k, coss[k])
    dev = _reference_bf16_deviation()
    tok_keys = [k for k in expect if k not in lnb_keys]
    med = float(np.median([worst[k] for k in tok_keys]))
    print(f"token-side median sample error {med:.4f} vs the reference's own bf16 deviation {dev['token_side']['sample_err_median']:.4f}")
    assert med <= 1.25 * dev["token_side"]["sample_err_median"] + 5e-3


def test_batchnorm_modes_agree_on_the_patch_model(gpu_device):
    """No BatchNorm layer: bn = "batch" (from_config's default) and "frozen" run the same step, bit for bit."""
    img, tok = synth.synth_images(3, seed=11).cuda(), synth.synth_tokens(3, seed=12).cuda()
    out = {}
    for bn in ("batch", "frozen"):
        m = _model()
        ts = train.from_config(m, named_config(NAME, BF16), bn=bn)
        loss = ts.forward(img, tok)
        out[bn] = (loss.item(), ts.backward())
    assert out["batch"][0] == out["frozen"][0]
    ga, gf = out["batch"][1], out["frozen"][1]
    assert sorted(ga) == sorted(gf) and len(ga) == 406
    for k in ga:
        if k == "token_embedding.weight":                                 # the scatter-add's fp32 atomics: order-dependent bits
            assert rel(ga[k], gf[k]) <= 1e-5, k
        else:
            assert torch.equal(ga[k], gf[k]), k


def test_training_loop_lowers_the_loss_l14(gpu_device):
    """from_config's AdamW (CUSTOM.LR_SHARE / WD_SHARE groups of the yaml) over two fixed batches: the loss falls."""
    m = _model()
    ts = train.from_config(m, named_config(NAME, BF16))
    ts.lr = ts.lr_share = 2e-5
    data = [(synth.synth_images(8, seed=10 + i).cuda(), synth.synth_tokens(8, seed=100 + i).cuda()) for i in range(2)]
    losses = []
    for step in range(8):
        losses.append(ts.forward(*data[step % 2]).item())
        ts.step(ts.backward())
    print("losses", losses)
    assert all(np.isfinite(losses)), losses
    assert max(losses[-2:]) < 0.5 * min(losses[:2]), losses
    assert np.isfinite(m.contrastive_loss(*data[0]).item())


@pytest.mark.parametrize("batch", [3, 5])
def test_training_step_odd_batches_l14(gpu_device, batch):
    m = _model()
    ts = train.from_config(m, named_config(NAME, BF16))
    img, tok = synth.synth_images(batch, seed=7).cuda(), synth.synth_tokens(batch, seed=8).cuda()
    loss = ts.forward(img, tok)
    grads = ts.backward()
    assert np.isfinite(loss.item()) and len(grads) == 406
    for k, gr in grads.items():
        assert bool(torch.isfinite(gr).all()), k
    before = m.visual.conv1.weight.detach().clone()
    ts.step(grads)
    assert not torch.equal(before, m.visual.conv1.weight.detach())


def test_checkpoint_resume_continues_the_run_l14(gpu_device, tmp_path):
    """Two steps, save, then the third once in the running process and once resumed from the file: bit for bit but for the
    two tables written by the embedding gradient's fp32 atomics (test_gpu_train.py::test_checkpoint_resume_continues_the_run)."""
    cfg = named_config(NAME, BF16)
    data = [(synth.synth_images(4, seed=20 + i).cuda(), synth.synth_tokens(4, seed=120 + i).cuda()) for i in range(3)]

    def run(ts, steps):
        for i in steps:
            ts.forward(*data[i])
            ts.step(ts.backward())
    mb = _model()
    tb = train.from_config(mb, cfg)
    run(tb, range(2))
    path = tmp_path / "checkpoint.pth"
    train.save_checkpoint(mb, tb, path, step=1, model_name=NAME)
    run(tb, [2])
    mc = _model()
    tc = train.from_config(mc, cfg)
    assert train.resume_checkpoint(mc, tc, path) == 2 and tc.steps == 2
    run(tc, [2])
    sb, sc = mb.state_dict(), mc.state_dict()
    atomics = ("token_embedding.weight", "positional_embedding")
    for k in sb:
        if k in atomics:
            assert rel(sc[k], sb[k]) <= 1e-5, (k, rel(sc[k], sb[k]))
        else:
            assert torch.equal(sb[k], sc[k]), (k, rel(sc[k].float(), sb[k].float()))
    k = "visual.conv1.weight"
    assert torch.equal(tc.state[k][0], tb.state[k][0]) and torch.equal(tc.state[k][1], tb.state[k][1]) and tc.steps == tb.steps == 3


@pytest.mark.parametrize("precision", ["fp8", "fp8-qkv"])
def test_fp8_training_of_the_patch_model_is_refused(gpu_device, precision):
    m = _model(precision)
    with pytest.raises(NotImplementedError, match="MODEL.SPEC.PRECISION bf16"):
        train.TrainStep(m, lr=1e-4)
