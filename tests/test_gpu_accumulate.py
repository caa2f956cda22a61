"""TrainStep.accumulate on a real MI355X: msclip_grad_accumulate, the K = 1 identity, every gradient element against the
oracle's autograd, the feature check and the BatchNorm state, accumulate + step end to end.

The gradient bounds are tests/gradcheck.py's, unchanged, with the r of tests/golden/train_full_gradient_ratios.json (measured
on the one-shot step): there is no tolerance of this file's own.  tools/accumulate_gradient_ratios.py writes the measured
engine / yardstick distributions of the same cases to tests/golden/accumulate_gradient_ratios.json, for information."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gradcheck as G
from accumulate_cases import CASES, build, case_id, chunks_of, run_case
from conftest import GOLDEN, ROOT
from msclip_amd import hip, synth, train
from train_full_cases import B32, L14

pytestmark = pytest.mark.gpu
TOK = "token_embedding.weight"
# Tensors allowed more than the class-worst bound, by name: {case id: {parameter: extra block error}} (none needed so far).
EXCEPTIONS = {}


def load_r():
    """r of tests/test_gpu_train_full.py: measured on the one-shot step, read, never re-derived here."""
    with open(os.path.join(GOLDEN, "train_full_gradient_ratios.json")) as f:
        d = json.load(f)
    assert 0 < d["r"] <= G.R_MAX and abs(d["r"] - min(G.R_MAX, 1.25 * d["measured_worst_ratio"])) < 1e-9
    return d["r"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------- the kernel
def test_grad_accumulate_kernel_is_bitwise_torch(gpu_device):
    """Modes 0 and 1 over one table of awkward tensors: a 0-d tensor, tiny and odd sizes, a piece boundary + 1, more than 40 M
    elements (several launches), views at element offsets that are not multiples of 4 (scalar path when acc and g disagree
    within 16 bytes, scalar head + 16-byte body when they agree).  Bitwise torch, guard elements around every accumulator
    untouched, three chunks = the left-to-right torch sum."""
    dev = gpu_device
    gen = torch.Generator(device="cpu").manual_seed(5)
    #        (elements, accumulator offset in elements within its slot, gradient offset in elements)
    specs = [((), 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (1023, 0, 0), (32768 + 1, 0, 0), (40_000_003, 0, 0),
             (1000, 0, 3), (1000, 1, 1), (70_001, 2, 3), (70_001, 3, 7), (6, 1, 1), (2, 3, 3)]
    GUARD = 16
    sizes = [1 if s == () else s for s, _, _ in specs]
    slots, total = [], 0
    for n, (_, ao, _) in zip(sizes, specs):
        total += GUARD
        slots.append(total + ao)
        total += (ao + n + 3) // 4 * 4 + GUARD
    SENT = 0x7FC12345                                      # a NaN pattern: any read-modify-write of a guard would still be caught bitwise
    arena = torch.full((total,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    accs = [arena[o:o + n].view(s if s == () else (n,)) for o, n, (s, _, _) in zip(slots, sizes, specs)]
    assert any(a.data_ptr() % 16 for a in accs)
    mask = torch.ones(total, dtype=torch.bool, device=dev)
    for o, n in zip(slots, sizes):
        mask[o:o + n] = False

    def fresh():
        out = []
        for n, (s, _, go) in zip(sizes, specs):
            base = torch.randn(n + go, generator=gen).to(dev)
            if n > 8:
                base[go + 1], base[go + 2], base[go + 5] = 1e-41, -0.0, 3e38        # a denormal, a signed zero, near overflow
            out.append(base[go:go + n].view(s if s == () else (n,)))
        return out
    plan = hip.AccumulatePlan(accs)
    g1, g2, g3 = fresh(), fresh(), fresh()
    assert any(g.data_ptr() % 16 for g in g1)
    plan.run(g1, 0)
    torch.cuda.synchronize()
    for a, g in zip(accs, g1):
        assert _same_bits(a, g), a.shape
    assert bool((arena.view(torch.int32)[mask] == SENT).all())
    plan.run(g2, 1)
    torch.cuda.synchronize()
    for a, x, y in zip(accs, g1, g2):
        assert _same_bits(a, x + y), a.shape
    plan.run(g3, 1)
    torch.cuda.synchronize()
    for a, x, y, z in zip(accs, g1, g2, g3):
        assert _same_bits(a, (x + y) + z), a.shape
    assert bool((arena.view(torch.int32)[mask] == SENT).all())
    # the gradients were only read
    gen2 = torch.Generator(device="cpu").manual_seed(5)
    assert _same_bits(g1[0], torch.randn(1, generator=gen2).to(dev).view(()))


# ---------------------------------------------------------------------------- K = 1
def _one_shot_and_k1(name, bn, batch):
    m, _ = build(name)
    img, tok = synth.synth_images(batch, seed=0).cuda(), synth.synth_tokens(batch, seed=1).cuda()
    bufs = {k: b.clone() for k, b in m.named_buffers()}
    ts = train.TrainStep(m, lr=1e-4, bn=bn)
    loss = ts.forward(img, tok)
    want = {k: g.clone() for k, g in ts.backward().items()}
    with torch.no_grad():
        for k, b in m.named_buffers():                       # (the running statistics the train-mode forward moved)
            b.copy_(bufs[k])
    loss2, got = ts.accumulate([(img, tok)])
    return loss, want, loss2, got


@pytest.mark.parametrize("name,bn,batch", [(B32, "frozen", 16), (B32, "batch", 16), (L14, "frozen", 4)],
                         ids=["b32-frozen", "b32-batch", "l14"])
def test_one_chunk_is_forward_plus_backward_bitwise(gpu_device, name, bn, batch):
    loss, want, loss2, got = _one_shot_and_k1(name, bn, batch)
    assert loss2.dim() == 0 and loss2.is_cuda and _same_bits(loss, loss2), (loss.item(), loss2.item())
    assert sorted(got) == sorted(want) and len(got) == (406 if name == L14 else 325)
    differ = [k for k in want if k != TOK and not _same_bits(want[k], got[k])]
    assert not differ, differ[:8]
    # token_embedding.weight: an atomic scatter-add (DESIGN s8) -- support and row bound of tests/gradcheck.py, against the one-shot result
    m = G.measure_one(TOK, got[TOK], want[TOK])
    print(f"{name} {bn}: {TOK} stray rows {m['stray_rows']}, worst row {m['row_err']:.3g}, block {m['block']:.3g}")
    assert m["stray_rows"] == 0 and m["row_err"] <= G.WORST_MARGIN and m["live_rows"] > 0


# ---------------------------------------------------------------------------- every element against the oracle
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_every_gradient_element_against_oracle_autograd(gpu_device, case):
    got, yard, loss, ref_loss, secs = run_case(case)
    cid = case_id(case)
    print(f"{cid}: loss {loss:.5f} (oracle {ref_loss:.5f}); oracle passes + metrics on the CPU {secs:.1f} s")
    print(G.describe(cid, got, yard))
    assert abs(loss - ref_loss) <= 2e-2, (loss, ref_loss)
    bad = G.violations(got, yard, load_r(), EXCEPTIONS.get(cid))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------- feature check, BatchNorm state
@pytest.mark.parametrize("bn", ["frozen", "batch"])
def test_feature_check_and_batchnorm_state(gpu_device, bn):
    m, _ = build(B32)
    img, tok = synth.synth_images(32, seed=0), synth.synth_tokens(32, seed=1)
    chunks = chunks_of(img, tok, (16, 16))
    ts = train.TrainStep(m, lr=1e-4, bn=bn)
    before = {k: b.clone() for k, b in m.named_buffers()}
    bank_i, bank_t, starts = ts._feature_pass(chunks)
    torch.cuda.synchronize()
    assert starts == [0, 16, 32] and bank_i.shape == bank_t.shape == (32, 1024) and bank_i.dtype == torch.bfloat16
    assert ts.saved is None                                  # nothing is kept for a backward
    changed = [k for k, b in m.named_buffers() if not torch.equal(b, before[k])]
    assert not changed, changed[:5]
    loss, grads = ts.accumulate(chunks, check_features=True)            # raises on the first chunk whose features differ
    assert torch.isfinite(loss) and len(grads) == 325
    moved = [k for k, b in m.named_buffers() if not torch.equal(b, before[k])]
    if bn == "frozen":
        assert not moved, moved[:5]
        return
    # the running statistics end where K ordinary train-mode forwards over the same chunks leave them
    m2, _ = build(B32)
    ts2 = train.TrainStep(m2, lr=1e-4, bn="batch")
    for c in chunks:
        ts2.forward(*c)
    b2 = dict(m2.named_buffers())
    assert moved and any(k.endswith("running_var") for k in moved) and any(k.endswith("num_batches_tracked") for k in moved)
    differ = [k for k, b in m.named_buffers() if not _same_bits(b.float(), b2[k].float())]
    assert not differ, differ[:5]
    # once per chunk: every counter that moved stands two above where it started (the synthetic state_dict does not start them at 0)
    counters = [k for k in moved if k.endswith("num_batches_tracked")]
    assert all(int(dict(m.named_buffers())[k]) == int(before[k]) + 2 for k in counters)


def test_returned_gradients_live_in_persistent_accumulators(gpu_device):
    m, _ = build(B32)
    img, tok = synth.synth_images(8, seed=0), synth.synth_tokens(8, seed=1)
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    _, g1 = ts.accumulate(chunks_of(img, tok, (4, 4)))
    where = {k: v.data_ptr() for k, v in g1.items()}
    snap = {k: v.clone() for k, v in g1.items()}
    _, g2 = ts.accumulate(chunks_of(img, tok, (3, 5)), clone=True)
    assert all(g2[k].data_ptr() != where[k] for k in where)                       # owned copies
    _, g3 = ts.accumulate(chunks_of(img, tok, (4, 4)))
    assert {k: v.data_ptr() for k, v in g3.items()} == where                      # stable addresses
    differ = [k for k in snap if k != TOK and not _same_bits(snap[k], g3[k])]     # and bitwise repeatable
    assert not differ, differ[:8]


# ---------------------------------------------------------------------------- end to end
def test_accumulate_then_step_equals_forward_backward_step(gpu_device):
    img, tok = synth.synth_images(16, seed=0).cuda(), synth.synth_tokens(16, seed=1).cuda()
    ma, _ = build(B32)
    ta = train.TrainStep(ma, lr=1e-4, bn="batch")
    ta.forward(img, tok)
    ta.step(ta.backward())
    mb, _ = build(B32)
    tb = train.TrainStep(mb, lr=1e-4, bn="batch")
    _, grads = tb.accumulate([(img, tok)])
    tb.step(grads)
    torch.cuda.synchronize()
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    differ = [k for k in pa if k != TOK and not _same_bits(pa[k].data, pb[k].data)]
    assert not differ, differ[:8]
    # token_embedding.weight: its gradient is an atomic sum, so the rows some caption touched agree to the row bound of
    # tests/gradcheck.py; the others (zero gradient on both sides) received the same update bit by bit
    t = G.measure_one(TOK, pb[TOK].data, pa[TOK].data)
    assert t["row_err"] <= G.WORST_MARGIN and t["stray_rows"] == 0
    untouched = torch.ones(pa[TOK].shape[0], dtype=torch.bool, device=img.device)
    untouched[tok.flatten().long()] = False
    assert bool(untouched.any()) and _same_bits(pa[TOK].data[untouched], pb[TOK].data[untouched])
    ba, bb = dict(ma.named_buffers()), dict(mb.named_buffers())
    assert all(_same_bits(ba[k].float(), bb[k].float()) for k in ba)
    # the engines' packed copies followed: the inference path (bf16 operands) agrees too, within the loss tolerance this suite
    # uses everywhere (2e-2, test_gpu_train_full.py) -- the two models differ in the rounding of token_embedding.weight only
    la, lb = float(ma.contrastive_loss(img, tok)), float(mb.contrastive_loss(img, tok))
    print(f"inference-path loss after one step: {la:.6f} / {lb:.6f}")
    assert abs(la - lb) <= 2e-2, (la, lb)


def test_train_synthetic_script_with_accumulate(gpu_device):
    """tools/train_synthetic.py --accumulate 4 --batch 16: six optimizer steps on 64-pair batches; its exit code is the
    check that the N-pair loss falls."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_synthetic.py"), "--accumulate", "4", "--batch", "16",
                        "--steps", "6"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "OK" in r.stdout and r.stdout.count("step ") == 6
    first = float(r.stdout.split("loss")[1].split()[0])
    assert first > 3.0, first                                # 64 pairs: ln 64 = 4.16 at chance, far above an in-chunk 16-pair loss (ln 16 = 2.77)


def test_more_than_one_process_is_refused(gpu_device, monkeypatch):
    from msclip_amd import comm as C
    m, _ = build(B32)
    ts = train.TrainStep(m, lr=1e-4)
    monkeypatch.setattr(type(C.comm), "collectives", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="single process"):
        ts.accumulate([(synth.synth_images(2, seed=0).cuda(), synth.synth_tokens(2, seed=1).cuda())])
