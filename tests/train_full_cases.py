"""The cases of tests/test_gpu_train_full.py and the code that runs one of them, shared with tools/train_full_gradient_ratios.py
(which measures r on them).  An ordinary helper module: no tests, no fixtures."""
import os
import time

import gradcheck as G
from conftest import GOLDEN, synth_sd
from msclip_amd import synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O
from oracle.autograd import oracle_gradients, parameter_aliases

B32, B16, L14 = "b32-yfcc-msclips", "b16-yfcc-msclips", "l14-fp8-msclips"
ARCH = {B32: O.arch_b32, B16: O.arch_b16, L14: O.arch_l14}
N_PARAMS = {B32: 325, B16: 325, L14: 406}
#        model, bn, batch, image seed, token seed
CASES = [(B32, "frozen", 32, 0, 1), (B32, "batch", 32, 0, 1), (B32, "frozen", 7, 7, 8), (B32, "batch", 7, 7, 8),
         (B16, "frozen", 4, 0, 1), (B16, "batch", 8, 0, 1), (L14, "frozen", 4, 0, 1)]
RATIOS = os.path.join(GOLDEN, "train_full_gradient_ratios.json")


def case_id(case):
    name, bn, batch, *_ = case
    return f"{name[:3]}-{bn}-b{batch}"


def run_case(case):
    """-> (measure(engine), measure(yardstick), engine loss, oracle loss, seconds spent in the oracle and the metrics)."""
    name, bn, batch, iseed, tseed = case
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(name), strict=True)
    alias = parameter_aliases(m)
    m = m.cuda().eval()
    img, tok = synth.synth_images(batch, seed=iseed), synth.synth_tokens(batch, seed=tseed)
    ts = train.TrainStep(m, lr=1e-4, bn=bn)
    loss = ts.forward(img.cuda(), tok.cuda()).item()
    grads = {k: g.detach().float().cpu() for k, g in ts.backward().items()}
    t0 = time.time()
    kw = dict(bn_train=bn == "batch", aliases=alias)
    ref, ref_loss = oracle_gradients(synth_sd(name), ARCH[name](), img, tok, **kw)
    yard, _ = oracle_gradients(synth_sd(name), ARCH[name](), img, tok, autocast_bf16=True, **kw)
    assert len(ref) == N_PARAMS[name]
    got, ym = G.measure(grads, ref), G.measure(yard, ref)
    return got, ym, loss, ref_loss, time.time() - t0
