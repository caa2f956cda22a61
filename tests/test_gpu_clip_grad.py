"""Gradient clipping by the global norm on a real MI355X: the norm kernels against fp64, the
clipped AdamW bit for bit against msclip_adamw_multi on gradients that torch multiplied by the device's own coefficient,
TrainStep(clip_grad_norm=...) on the B/32 and L/14 models, and accumulate() followed by a clipped step.

Reference: torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) + torch.optim.AdamW.

The norm's bound (1e-5 relative, derived, not measured): a term of the sum of squares passes through at most 43 fp32 roundings
inside a workgroup (clip.hip: <= 32 fmaf per accumulator, 2 to fold a thread's four accumulators, 1 head / tail element, 6
shuffle steps, 2 over the four waves); all terms are non-negative, so the relative error of a chunk's partial is at most
43 * 2^-24 = 2.6e-6; the fold over the partials is in double.  The norm, a square root, carries half of that plus the
roundings of the final fp32 conversion: 1.4e-6.  1e-5 is the bound of the 140-addition shape (128 serial additions per thread)
that this kernel's shape stays inside."""
import ctypes

import pytest
import torch

from conftest import synth_sd
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B32, L14 = "b32-yfcc-msclips", "l14-fp8-msclips"
NORM_TOL = 1e-5
# 1 ... 768 * 768: below, at and above the 32 K chunk; 13 200 003: 403 chunks, more than one launch's chunk map (400); 60 small
# tensors on top: more than one launch's tensor table (36)
SIZES = [1, 3, 768, 32767, 32768, 32769, 3 * 32768 + 12, 768 * 768, 13_200_003] + [100 + 7 * i for i in range(60)]
ZERO = 1                                                     # the tensor that is all zeros


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def rel(got, ref):
    return ((got.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-12)).item()


def _norm64(tensors):
    return float(torch.sqrt(sum(t.double().pow(2).sum() for t in tensors)))


@pytest.fixture(scope="module")
def ragged(gpu_device):
    """(flat buffer, [gradient views at odd 4-byte offsets], fp64 norm): randn times a per-tensor scale in [1e-3, 1e2], one
    tensor all zeros.  Shared by the kernel-level tests, which leave it unchanged."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    flat = torch.randn(sum(SIZES) + len(SIZES) + 1, device="cuda", generator=gen)
    gs, o = [], 1
    for i, n in enumerate(SIZES):
        g = flat[o:o + n]
        g *= 0.0 if i == ZERO else 10.0 ** (-3.0 + 5.0 * ((i * 7) % len(SIZES)) / (len(SIZES) - 1))
        gs.append(g)
        o += n + 1
    assert any(g.data_ptr() % 16 for g in gs) and any(g.data_ptr() % 16 == 0 for g in gs) and not bool(gs[ZERO].any())
    return flat, gs, _norm64(gs)


def _raw_norm(gs, max_norm, partials=None):
    """msclip_grad_sumsq + msclip_clip_coef through the bound library on a caller-filled partials array -> {norm, coef} tensor."""
    arr = (hip.SumsqTensor * len(gs))()
    for q, g in zip(arr, gs):
        q.g, q.n = g.data_ptr(), g.numel()
    n_partials = sum((g.numel() + hip.CLIP_CHUNK - 1) // hip.CLIP_CHUNK for g in gs)
    if partials is None:
        partials = torch.full((n_partials + 3,), float("nan"), device="cuda")
    out = torch.full((4,), 7.0, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.lib().msclip_grad_sumsq(arr, len(gs), ctypes.c_void_p(partials.data_ptr()), n_partials, st) == 0
    assert hip.lib().msclip_clip_coef(ctypes.c_void_p(partials.data_ptr()), n_partials, max_norm, ctypes.c_void_p(out.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(partials[n_partials:]).all()) and bool((out[2:] == 7.0).all())      # nothing written past the ends
    return out[:2], partials[:n_partials]


# ---------------------------------------------------------------------------- 2. the norm kernels against fp64
def test_norm_of_a_ragged_list_against_fp64(ragged):
    flat, gs, n64 = ragged
    assert sum((n + 32767) // 32768 for n in SIZES) > 400 + 60 and len(SIZES) > 36
    out, partials = _raw_norm(gs, 1.0)                                 # the partials array starts as NaN: every slot is written
    assert bool(torch.isfinite(partials).all())
    err = abs(out[0].item() - n64) / n64
    print(f"norm {out[0].item():.9g}  fp64 {n64:.12g}  relative error {err:.3g}  (bound {NORM_TOL:g})")
    assert err <= NORM_TOL
    assert abs(out[1].item() - 1.0 / (n64 + 1e-6)) <= NORM_TOL * (1.0 / n64)
    again, partials2 = _raw_norm(gs, 1.0)                              # fixed addition order: bitwise repeatable
    assert _same_bits(out, again) and _same_bits(partials, partials2)
    assert _same_bits(hip.grad_norm(gs), out[0])                       # the helper is the same two calls
    n2, c2 = hip.grad_norm(gs, max_norm=1.0)
    assert _same_bits(n2, out[0]) and _same_bits(c2, out[1])
    # single tensors: one element, a chunk minus / plus one, at every alignment of the first element
    for i in (0, 3, 4, 5, 6):
        for shift in range(4):
            t = flat[9 + shift:9 + shift + SIZES[i]]
            want = _norm64([t])
            got = hip.grad_norm([t]).item()
            assert abs(got - want) <= NORM_TOL * want, (SIZES[i], shift, got, want)
    assert hip.grad_norm([gs[ZERO]]).item() == 0.0 and hip.grad_norm([gs[ZERO]], max_norm=3.0)[1].item() == 1.0


def test_nan_and_inf_reach_norm_and_coefficient(ragged):
    _, gs, _ = ragged
    for bad, where in ((float("nan"), 7), (float("inf"), 8), (float("-inf"), 3)):
        mine = [g.clone() for g in gs[:12]]
        mine[where].view(-1)[mine[where].numel() // 2] = bad
        ref = [g.clone().requires_grad_(True) for g in mine]
        for r, g in zip(ref, mine):
            r.grad = g.clone()
        want = torch.nn.utils.clip_grad_norm_(ref, 2.0, error_if_nonfinite=False)
        norm, coef = hip.grad_norm(mine, max_norm=2.0)
        if bad != bad:
            assert bool(torch.isnan(norm)) and bool(torch.isnan(coef)) and bool(torch.isnan(want))
        else:
            assert norm.item() == float("inf") == want.item() and coef.item() == 0.0


# ---------------------------------------------------------------------------- 3. coefficient and clipped AdamW, kernel level
KINDS = {2: (BF, 0.125), 6: (BF, 1.0), 7: (torch.float32, 0.125), 8: (BF, 0.125), 11: (torch.float32, 1.0), 40: (BF, 1.0)}
GUARD = 4


def _rates(n):
    return 1e-3 * (1 + n % 3), 0.2 * (n % 2)


def _state(ps):
    return [(p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]


def _packs():
    return {i: torch.full((SIZES[i] + 8,), 7.0, dtype=dt, device="cuda") for i, (dt, _) in KINDS.items()}


def _items(state, gs, pks):
    out = []
    for i, ((p, m, v), g) in enumerate(zip(state, gs)):
        n = SIZES[i]
        pk = pks.get(i)
        out.append((p[:n], g, m[:n], v[:n], *_rates(n), None if pk is None else pk[:n], KINDS[i][1] if pk is not None else 1.0))
    return out


def _assert_same(a, b, pa, pb, what):
    for i, ((p1, m1, v1), (p2, m2, v2)) in enumerate(zip(a, b)):
        assert _same_bits(p1, p2) and _same_bits(m1, m2) and _same_bits(v1, v2), (what, SIZES[i], (p1 - p2).abs().max().item())
    for i in pa:
        assert torch.equal(pa[i], pb[i]), (what, "packed copy", SIZES[i])


@pytest.fixture(scope="module")
def params(ragged):
    gen = torch.Generator(device="cuda").manual_seed(6)
    return [torch.randn(n + GUARD, device="cuda", generator=gen) for n in SIZES]


def test_loose_max_norm_is_the_unclipped_kernel_bit_for_bit(ragged, params):
    flat, gs, n64 = ragged
    plain, loose = _state(params), _state(params)
    pk_plain, pk_loose = _packs(), _packs()
    ref_plan = hip.AdamwPlan(_items(plain, gs, pk_plain))
    plan = hip.AdamwPlan(_items(loose, gs, pk_loose))
    plan.partials.fill_(float("nan"))
    for step in (1, 2, 3):
        fs = flat * step                                               # this step's gradients: new addresses, same offsets
        sg = [fs[g.storage_offset():g.storage_offset() + g.numel()] for g in gs]
        ref_plan.set_grads([g.data_ptr() for g in sg])
        plan.set_grads([g.data_ptr() for g in sg])
        ref_plan.run(0.9, 0.98, 1e-6, step)
        plan.run(0.9, 0.98, 1e-6, step, max_norm=2.0 * step * n64)
        assert plan.coef.item() == 1.0 and abs(plan.norm.item() - step * n64) <= NORM_TOL * step * n64
    _assert_same(plain, loose, pk_plain, pk_loose, "max_norm = 2 norm")
    assert not _same_bits(plain[7][0], params[7])


def test_clipped_adamw_is_adamw_on_gradients_scaled_by_the_device_coefficient(ragged, params):
    flat, gs, n64 = ragged
    scaled, clipped = _state(params), _state(params)
    pk_scaled, pk_clipped = _packs(), _packs()
    ref_plan = hip.AdamwPlan(_items(scaled, gs, pk_scaled))
    plan = hip.AdamwPlan(_items(clipped, gs, pk_clipped))
    plan.partials.fill_(float("nan"))
    tp = [p[:n].clone().requires_grad_(True) for p, n in zip(params, SIZES)]
    opt = torch.optim.AdamW([dict(params=[t], lr=_rates(n)[0], weight_decay=_rates(n)[1]) for t, n in zip(tp, SIZES)],
                            betas=(0.9, 0.98), eps=1e-6)
    for step in (1, 2, 3):
        fs = flat * step
        sg = [fs[g.storage_offset():g.storage_offset() + g.numel()] for g in gs]
        max_norm = 0.5 * step * n64
        plan.set_grads([g.data_ptr() for g in sg])
        plan.run(0.9, 0.98, 1e-6, step, max_norm=max_norm)
        coef = plan.coef.clone()                                       # the device's own fp32 coefficient
        want = max_norm / (step * n64 + 1e-6)
        assert abs(coef.item() - want) <= 1e-5 * want, (coef.item(), want)
        pre = fs * coef                                                # ONE torch fp32 multiply per element
        ref_plan.set_grads([pre[g.storage_offset():].data_ptr() for g in gs])
        ref_plan.run(0.9, 0.98, 1e-6, step)
        assert torch.equal(fs, flat * step)                            # the clipped step wrote no gradient
        for t, g in zip(tp, sg):
            t.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
    _assert_same(scaled, clipped, pk_scaled, pk_clipped, "max_norm = norm / 2")
    for i, ((p, m, v), p0) in enumerate(zip(clipped, params)):
        n = SIZES[i]
        assert _same_bits(p[n:], p0[n:]) and not bool(m[n:].any()) and not bool(v[n:].any()), ("guard", n)
        assert not _same_bits(p[:n], p0[:n])
        err = rel(p[:n], tp[i].detach())
        assert err < 1e-5, (n, err)
    for i, pk in pk_clipped.items():
        n = SIZES[i]
        assert torch.equal(pk[:n], (clipped[i][0][:n] * KINDS[i][1]).to(pk.dtype)) and bool((pk[n:] == 7.0).all()), n


def test_clipped_calls_reject_bad_arguments(gpu_device):
    p, g = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda")
    plan = hip.AdamwPlan([(p, g, torch.zeros_like(p), torch.zeros_like(p), 1e-3, 0.0)])
    with pytest.raises(hip.HipError):
        plan.run(0.9, 0.999, 1e-8, 0, max_norm=1.0)                    # step < 1
    with pytest.raises(hip.HipError):
        plan.run(0.9, 0.999, 1e-8, 1, max_norm=-1.0)
    with pytest.raises(ValueError):
        hip.grad_norm([p[:0]])
    plan.run(0.9, 0.999, 1e-8, 1, max_norm=1.0)
    assert abs(plan.norm.item() - 8 ** 0.5) < 1e-6 and abs(plan.coef.item() - 1 / (8 ** 0.5 + 1e-6)) < 1e-6


# ---------------------------------------------------------------------------- 4. the training step
def _fresh(name):
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(name), strict=True)
    return m.cuda().eval()


def _snapshot(m, ts):
    """Everything a step writes: parameters, both moments, the engine's bf16 / fp32 copies of the blocks' projections."""
    out = {"p/" + k: p.detach().clone() for k, p in m.named_parameters()}
    for k, (mom, var) in ts.state.items():
        out["m/" + k], out["v/" + k] = mom.clone(), var.clone()
    e = ts.eng
    for blocks in ("tblk", "vblk"):
        for i, b in enumerate(getattr(e, blocks)):
            if b is not None:
                for f in ("wqkv", "bqkv", "wo", "bo", "wfc", "bfc", "wpr", "bpr"):
                    out[f"e/{blocks}{i}.{f}"] = getattr(b["w"], f).clone()
    return out


def _differ(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not _same_bits(a[k], b[k])]


@pytest.fixture(scope="module")
def b32_grads(gpu_device):
    """One backward of the B/32 model at batch 8 (frozen statistics): (owned gradients, their fp64 norm).  Every model below is
    built identically and stepped on THESE tensors, so bitwise comparisons hold (token_embedding.weight's atomic sums included)."""
    m = _fresh(B32)
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    ts.forward(synth.synth_images(8, seed=51).cuda(), synth.synth_tokens(8, seed=52).cuda())
    grads = ts.backward(clone=True)
    ts.saved = None
    assert len(grads) == 325 and "logit_scale" in grads
    return grads, _norm64(grads.values())


_CACHE = {}


def _scaled_reference(b32_grads):
    """The unclipped step on gradients multiplied in torch by model A's own coefficient (and A's results), computed once."""
    if "ref" not in _CACHE:
        grads, N = b32_grads
        before = {k: g.clone() for k, g in grads.items()}
        ma = _fresh(B32)
        ta = train.TrainStep(ma, lr=1e-4, bn="frozen", clip_grad_norm=0.5 * N)
        assert ta.last_grad_norm is None and ta.last_clip_coef is None
        ta.step(grads)
        norm, coef = ta.last_grad_norm, ta.last_clip_coef
        assert norm.dim() == 0 and coef.dim() == 0 and norm.is_cuda and coef.is_cuda
        assert all(_same_bits(before[k], grads[k]) for k in grads)     # nothing written back
        mb = _fresh(B32)
        tb = train.TrainStep(mb, lr=1e-4, bn="frozen")
        tb.step({k: g * coef for k, g in grads.items()})               # a single torch fp32 multiply per element
        assert tb.last_grad_norm is None
        _CACHE["ref"] = (_snapshot(ma, ta), _snapshot(mb, tb), norm.item(), coef.item())
    return _CACHE["ref"]


def test_clipped_training_step_is_the_unclipped_step_on_scaled_gradients(b32_grads):
    _, N = b32_grads
    a, b, norm, coef = _scaled_reference(b32_grads)
    print(f"B/32 batch 8: fp64 norm {N:.9g}, device norm {norm:.9g} (relative error {abs(norm - N) / N:.3g}), coef {coef:.9g}")
    assert abs(norm - N) <= NORM_TOL * N
    want = 0.5 * N / (N + 1e-6)
    assert abs(coef - want) <= 1e-5 * want
    assert any(k.startswith("e/") for k in a) and any(k.startswith("m/") for k in a)
    assert not _differ(a, b), _differ(a, b)[:8]


def test_loose_clip_grad_norm_is_the_unclipped_training_step(b32_grads):
    grads, N = b32_grads
    mc, md = _fresh(B32), _fresh(B32)
    tc = train.TrainStep(mc, lr=1e-4, bn="frozen", clip_grad_norm=2.0 * N)
    td = train.TrainStep(md, lr=1e-4, bn="frozen", clip_grad_norm=0.0)                     # 0.0: off
    tc.step(grads)
    td.step(grads)
    assert tc.last_clip_coef.item() == 1.0 and abs(tc.last_grad_norm.item() - N) <= NORM_TOL * N
    assert td.last_clip_coef is None and td.last_grad_norm is None
    c, d = _snapshot(mc, tc), _snapshot(md, td)
    assert not _differ(c, d), _differ(c, d)[:8]


def test_from_config_reads_clip_grad_norm(b32_grads):
    grads, N = b32_grads
    a, _, norm, coef = _scaled_reference(b32_grads)
    cfg = named_config(B32, ["TRAIN.CLIP_GRAD_NORM", str(0.5 * N)])
    assert train.from_config(_fresh(B32), named_config(B32)).clip_grad_norm == 0.0
    me = _fresh(B32)
    te = train.from_config(me, cfg, bn="frozen")
    assert te.clip_grad_norm == 0.5 * N
    te.lr_share = te.wd_share = None                                   # model A's groups: TrainStep(lr=1e-4), the yaml's TRAIN.LR
    assert te.lr == 1e-4 and te.wd == 0.05
    te.step(grads)
    assert te.last_grad_norm.item() == norm and te.last_clip_coef.item() == coef
    e = _snapshot(me, te)
    assert not _differ(a, e), _differ(a, e)[:8]


def test_clipped_training_step_on_the_l14_model(gpu_device):
    m = _fresh(L14)
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    ts.forward(synth.synth_images(3, seed=7).cuda(), synth.synth_tokens(3, seed=8).cuda())
    grads = ts.backward()
    assert len(grads) == 406
    N = _norm64(grads.values())
    ts.clip_grad_norm = 0.5 * N
    ts.step(grads)
    norm, coef = ts.last_grad_norm.item(), ts.last_clip_coef.item()
    print(f"L/14 batch 3: fp64 norm {N:.9g}, device norm {norm:.9g} (relative error {abs(norm - N) / N:.3g}), coef {coef:.9g}")
    want = 0.5 * N / (N + 1e-6)
    assert abs(norm - N) <= NORM_TOL * N and abs(coef - want) <= 1e-5 * want


# ---------------------------------------------------------------------------- 5. accumulate
def test_accumulate_then_clipped_step(gpu_device):
    m = _fresh(B32)
    img, tok = synth.synth_images(8, seed=0).cuda(), synth.synth_tokens(8, seed=1).cuda()
    ts = train.TrainStep(m, lr=2e-5, bn="frozen")
    chunks = [(img[:4], tok[:4]), (img[4:], tok[4:])]
    loss0, grads = ts.accumulate(chunks)
    # the norm of the SUM over the chunks, over whole gradient tensors in the optimizer's order: the same chunks, the same order
    want = hip.grad_norm([grads[k].reshape(-1) for k, *_ in ts.param_groups() if k in grads])
    N = _norm64(grads.values())
    ts.clip_grad_norm = 0.5 * N
    ts.step(grads)
    assert _same_bits(ts.last_grad_norm, want) and abs(want.item() - N) <= NORM_TOL * N
    assert ts.last_clip_coef.item() < 0.51
    loss1, _ = ts.accumulate(chunks)
    assert loss1.item() < loss0.item(), (loss0.item(), loss1.item())
