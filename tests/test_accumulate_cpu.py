"""TrainStep.accumulate's contract has teeth, and msclip_grad_accumulate validates its arguments (no GPU needed).

ViT-B/32, 32 pairs (synth_images(32, seed=0) / synth_tokens(32, seed=1)).  The reference of the N-pair step is the oracle's
autograd -- on the whole batch with frozen statistics, chunk by chunk (tests/accumulate_ref.py) with train-mode BatchNorm --
and the stand-in for a correct bf16 implementation is the same under bf16 autocast, as in tests/test_gradcheck_cpu.py.  Each
way of getting gradient accumulation wrong must be reported by gradcheck.violations at the r that the GPU tests use
(tests/golden/train_full_gradient_ratios.json); the correct reference must produce no violation."""
import json
import os

import pytest
import torch

import gradcheck as G
from accumulate_ref import chunked_oracle_gradients, in_chunk_mean
from conftest import GOLDEN, synth_sd
from msclip_amd import hip, synth
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O
from oracle.autograd import oracle_gradients, parameter_aliases

NAME, BATCH = "b32-yfcc-msclips", 32


def load_r():
    with open(os.path.join(GOLDEN, "train_full_gradient_ratios.json")) as f:
        return json.load(f)["r"]


@pytest.fixture(scope="module")
def model():
    m = get_clip_model(named_config(NAME))
    m.load_state_dict(synth_sd(NAME), strict=True)
    return m


@pytest.fixture(scope="module")
def data():
    return synth.synth_images(BATCH, seed=0), synth.synth_tokens(BATCH, seed=1)


@pytest.fixture(scope="module")
def frozen(model, data):
    """Frozen statistics: (reference, its loss, measure(yardstick)) of the one-shot step on all 32 pairs."""
    img, tok = data
    ref, loss = oracle_gradients(model, O.arch_b32(), img, tok)
    yard, _ = oracle_gradients(model, O.arch_b32(), img, tok, autocast_bf16=True)
    return ref, loss, G.measure(yard, ref)


@pytest.fixture(scope="module")
def per_chunk(model, data):
    """Train-mode BatchNorm at 2 x 16: (reference, its loss, measure(yardstick)) from the per-chunk helper."""
    img, tok = data
    ref, loss = chunked_oracle_gradients(model, O.arch_b32(), img, tok, [16, 16], bn_train=True)
    yard, _ = chunked_oracle_gradients(model, O.arch_b32(), img, tok, [16, 16], bn_train=True, autocast_bf16=True)
    return ref, loss, G.measure(yard, ref)


def _report(what, got, ym):
    bad = G.violations(got, ym, load_r())
    print(f"{what}: {len(bad)} violations; first: {bad[:3]}")
    return bad


def test_per_chunk_helper_at_one_chunk_is_oracle_gradients(model):
    img, tok = synth.synth_images(8, seed=0), synth.synth_tokens(8, seed=1)
    a, la = chunked_oracle_gradients(model, O.arch_b32(), img, tok, [8], bn_train=True)
    b, lb = oracle_gradients(model, O.arch_b32(), img, tok, bn_train=True)
    assert sorted(a) == sorted(b) and len(a) == 325
    worst = max(float((a[k] - b[k]).abs().max()) for k in a)
    print(f"one chunk against oracle_gradients(bn_train=True): max difference {worst:.3g}, loss {la} / {lb}")
    assert la == lb and worst <= 1e-6


def test_correct_reference_produces_no_violation(model, data, frozen, per_chunk):
    ref, loss, ym = frozen
    assert len(ref) == 325
    assert G.violations(ym, ym, load_r()) == []
    # frozen statistics: chunking the image tower changes nothing (the step is the one-shot step on the concatenated batch)
    chunked, closs = chunked_oracle_gradients(model, O.arch_b32(), *data, [8, 8, 8, 8])
    assert abs(closs - loss) <= 1e-5
    assert _report("chunked 4 x 8 reference against the one-shot reference", G.measure(chunked, ref), ym) == []
    ref2, _, ym2 = per_chunk
    assert G.violations(ym2, ym2, load_r()) == []
    assert G.violations(G.measure(ref2, ref2), ym2, load_r()) == []


def test_in_chunk_negatives_are_reported(model, data, frozen):
    """The sum of K ordinary steps (divided by K): every pair against the 7 negatives of its own chunk, not all 31."""
    ref, loss, ym = frozen
    mean, mloss = in_chunk_mean(model, O.arch_b32(), *data, [8, 8, 8, 8])
    print(f"loss over all 32 pairs {loss:.4f}, mean of the four 8-pair losses {mloss:.4f}")
    assert mloss < loss - 1.0
    bad = _report("in-chunk negatives only (mean of four 8-pair gradients)", G.measure(mean, ref), ym)
    assert bad


def test_whole_batch_statistics_are_reported(model, data, per_chunk):
    """BatchNorm over all 32 images at once where the contract says per chunk of 16."""
    ref, _, ym = per_chunk
    whole, _ = oracle_gradients(model, O.arch_b32(), *data, bn_train=True)
    bad = _report("whole-batch BatchNorm statistics against the per-chunk reference at 2 x 16", G.measure(whole, ref), ym)
    assert bad


def test_dropped_chunk_and_mean_instead_of_sum_are_reported(model, data, frozen):
    ref, _, ym = frozen
    dropped, _ = chunked_oracle_gradients(model, O.arch_b32(), *data, [8, 8, 8, 8], live_chunks=(0, 1, 3))
    bad = _report("the third chunk's gradient dropped", G.measure(dropped, ref), ym)
    assert bad
    bad = _report("the sum divided by K = 4", G.measure({k: v / 4 for k, v in ref.items()}, ref), ym)
    assert bad


def test_grad_accumulate_validates_on_the_host():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
    # host-side argument validation, before any launch
    one = (hip.AccumTensor * 1)()
    assert L.msclip_grad_accumulate(None, 1, 0, None) == -1 and L.msclip_grad_accumulate(one, 1, 0, None) == -1
    one[0].acc, one[0].g, one[0].n = 4096, 8192, 16
    assert L.msclip_grad_accumulate(one, 1, 2, None) == -1 and L.msclip_grad_accumulate(one, -1, 0, None) == -1
    one[0].g = 8193                                          # not 4-byte aligned
    assert L.msclip_grad_accumulate(one, 1, 1, None) == -1


def test_accumulate_refuses_more_than_one_process(monkeypatch):
    """No hardware exists to test chunks composed with ranks: the call says so before touching the GPU."""
    from msclip_amd import comm as C, train
    ts = train.TrainStep.__new__(train.TrainStep)            # the refusal comes first: no engine, no device needed
    ts.dev = torch.device("cpu")
    monkeypatch.setattr(type(C.comm), "collectives", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="single process"):
        ts.accumulate([(None, None)])
