"""The oracle's autograd IS the reference's (no GPU needed).

oracle/autograd.py::oracle_gradients against every gradient fixture captured from autograd of the real reference
(tests/golden/*.grads*.npz, tools/make_golden.py::grads_fixture), eval-mode and train-mode BatchNorm, three models, batches
4 / 8 / 16 / 32: the loss, every stored 64-point sample and abs-mean, every tensor stored in full, and the key set.  This is what
licenses tests/test_gpu_train_full.py to take the oracle as the reference for the 99.85 % of the gradient elements that the
fixtures do not hold.

Bounds: twice what was measured when this test was written (16 threads; the factor covers thread counts and summation
orders) -- eval-mode B/32 and B/16: worst sample error 1.96e-3 / 1.38e-3 / 1.98e-3 of abs-max, all on
parallel_branch_v.3...bn2.weight (a per-channel sum over the map of nearly cancelling fp32 terms), lowest cosine 0.999999;
train-mode BatchNorm and L/14: <= 1.4e-5.  (Eval mode is the noisier one because the oracle's eval-mode BatchNorm is the folded
x * scale + shift of the inference path: with eps = 1e-6 the parallel branch's scales are large, a last-bit difference in a
map flips ReLU masks downstream, and per-channel gradients there are sums of nearly cancelling terms.)"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, summarize, synth_sd
from msclip_amd import synth
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O
from oracle.autograd import oracle_gradients, parameter_aliases

B32, B16, L14 = "b32-yfcc-msclips", "b16-yfcc-msclips", "l14-fp8-msclips"
ARCH = {B32: O.arch_b32, B16: O.arch_b16, L14: O.arch_l14}
#          model, fixture tag,      train-mode BN, sample bound, cosine bound, parameters
FIXTURES = [(B32, "grads", False, 4e-3, 0.99999, 325),
            (B32, "grads_b32", False, 4e-3, 0.99999, 325),
            (B32, "grads_trainbn", True, 1e-4, 0.99999, 325),
            (B32, "grads_trainbn_b32", True, 1e-4, 0.99999, 325),
            (B16, "grads", False, 4e-3, 0.99999, 325),
            (B16, "grads_trainbn", True, 1e-4, 0.99999, 325),
            (L14, "grads", False, 1e-4, 0.99999, 406)]


def cpu_model(name):
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(name), strict=True)
    return m


@pytest.mark.parametrize("name,tag,bn_train,sample_tol,cos_tol,n_params", FIXTURES, ids=[f"{f[0][:3]}-{f[1]}" for f in FIXTURES])
def test_oracle_autograd_is_the_reference_autograd(name, tag, bn_train, sample_tol, cos_tol, n_params):
    g = np.load(os.path.join(GOLDEN, f"{name}.{tag}.npz"))
    b, seed = int(g["batch"]), int(g["seed"])
    m = cpu_model(name)
    grads, loss = oracle_gradients(m, ARCH[name](), synth.synth_images(b, seed=seed), synth.synth_tokens(b, seed=seed + 1), bn_train=bn_train)
    assert abs(loss - float(g["loss"])) <= 1e-5, (loss, float(g["loss"]))
    expect = sorted(k[2:] for k in g.files if k.startswith("g_"))
    assert sorted(grads) == expect and len(expect) == n_params
    # the text-tower names of the shared tensors resolve to the name their gradient is stored under, as in the fixture
    alias = parameter_aliases(m)
    assert {k: v for k, v in alias.items() if k != v} == {k[6:]: str(g[k]) for k in g.files if k.startswith("alias_")}
    sample, absmean, full_err, cos = {}, {}, {}, {}
    for k in expect:
        sm, ref = summarize(grads[k]), g["g_" + k]
        scale = max(float(g["gmax_" + k]), 1e-30)
        sample[k] = float(np.abs(sm[2:] - ref[2:]).max() / scale)
        absmean[k] = float(abs(sm[1] - ref[1]) / (ref[1] + 1e-30))
        if "gfull_" + k in g.files:
            full = torch.from_numpy(g["gfull_" + k])
            assert full.shape == grads[k].shape, k
            full_err[k] = float((grads[k] - full).abs().max() / scale)
            if full.numel() > 1:
                cos[k] = F.cosine_similarity(grads[k].flatten().double(), full.flatten().double(), dim=0).item()
    ws, wa, wf, wc = max(sample, key=sample.get), max(absmean, key=absmean.get), max(full_err, key=full_err.get), min(cos, key=cos.get)
    print(f"{name} {tag}: loss {loss:.6f} (fixture {float(g['loss']):.6f}) | worst sample error / abs-max {sample[ws]:.3e} {ws} | worst abs-mean "
          f"deviation {absmean[wa]:.3e} {wa} | {len(full_err)} tensors in full: worst error / abs-max {full_err[wf]:.3e} {wf}, lowest cosine "
          f"{cos[wc]:.7f} {wc}")
    for k in expect:
        assert sample[k] <= sample_tol, (k, sample[k])
        assert absmean[k] <= sample_tol, (k, absmean[k])
    for k in full_err:
        # the largest of all n elements instead of the largest of 64 of them: with the same error per element the expected
        # maximum of n draws grows like sqrt(2 ln n), so the sample bound is scaled by sqrt(ln n / ln 64) (1.41 at n = 4096;
        # measured worst 4.4e-3 against 5.0e-3 at n = 768, parallel_branch_v.3...bn3.bias of ViT-B/16 in eval mode)
        n = max(grads[k].numel(), 64)
        assert full_err[k] <= sample_tol * float(np.sqrt(np.log(n) / np.log(64))), (k, full_err[k])
    for k in cos:
        assert cos[k] >= cos_tol, (k, cos[k])


def test_eval_mode_stays_the_default_and_train_mode_uses_batch_statistics():
    """Arch.bn_train is off by default; switched on, batch_norm normalises with the batch's own mean and BIASED variance and does
    not read the running statistics."""
    assert O.Arch().bn_train is False and O.arch_b16().bn_train is False
    x = torch.randn(5, 7, 6, 6, generator=torch.Generator().manual_seed(0)) * 3 + 1
    sd = {"bn.weight": torch.rand(7) + 0.5, "bn.bias": torch.randn(7), "bn.running_mean": torch.full((7,), 1e3), "bn.running_var": torch.full((7,), 1e-3)}
    y = O.batch_norm(x, sd, "bn", 1e-5, True)
    mu, var = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
    want = (x - mu) / torch.sqrt(var + 1e-5) * sd["bn.weight"][None, :, None, None] + sd["bn.bias"][None, :, None, None]
    assert (y - want).abs().max().item() <= 1e-5
    ev = O.batch_norm(x, sd, "bn", 1e-5)
    scale = sd["bn.weight"] / torch.sqrt(sd["bn.running_var"] + 1e-5)
    assert torch.equal(ev, x * scale[None, :, None, None] + (sd["bn.bias"] - sd["bn.running_mean"] * scale)[None, :, None, None])
