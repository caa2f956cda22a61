"""TRAIN.OPTIMIZER lamb on a real MI355X: the norm and ratio kernels against fp64, the apply pass bit for bit against
msclip_adamw_multi handed the device's own scaled rates, trust_clip, non-finite gradients, and TrainStep(optimizer="lamb") on
the B/32 model against tests/lamb_ref.py, with clipping, EMA, accumulate(), the schedule and a checkpoint round trip.

Bounds (derived, not measured).  ||w||: 1e-5 relative, the bound tests/test_gpu_clip_grad.py derives for this reduction shape
(<= 43 roundings on the path of a term, 2.6e-6 for a chunk's partial, the fold over the partials in double).  ||u||: 1e-5 * N
with N = sqrt(sum (|a_i| + |wd w_i|)^2), a = m_hat / (sqrt(v_hat) + eps): about 8 fp32 operations of <= 1 ulp per element of u
(the moments, the bias corrections, a square root, a reciprocal, the products, the final fma) on top of the reduction's 2.6e-6,
stated against N so that it holds when a and wd w cancel.  The ratio: both, combined to first order, plus its own division.
The training step: |w_new - w_ref| <= 2^-23 |w| + 3e-5 max|delta_ref| per tensor -- the rounding of the fp32 store, the ratio's
bound and the element-wise error of u."""
import ctypes

import numpy as np
import pytest
import torch

import gradcheck as G
import lamb_ref as R
from conftest import synth_sd
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
B32 = "b32-yfcc-msclips"
TOK = "token_embedding.weight"
NORM_TOL = 1e-5
CHUNK = 32768
# test_gpu_clip_grad.py's list, for its reasons: below, at and above the 32 K chunk; 13 200 003: 403 chunks, more than one launch's
# chunk map (400); 60 small tensors on top: more than one launch's tensor table (32)
SIZES = [1, 3, 768, 32767, 32768, 32769, 3 * 32768 + 12, 768 * 768, 13_200_003] + [100 + 7 * i for i in range(60)]
ZERO = 1                                                     # the parameter whose weight is all zeros (wd = 0.2: it adapts)
SPLIT, SPLIT_AT = 7, 768 * 256                               # the parameter that is two adjacent items (in_proj_weight's q rows | k, v rows)
KINDS = {2: (BF, 0.125), 6: (BF, 1.0), 8: (F32, 0.125), 11: (F32, 1.0), 40: (BF, 1.0)}
SPLIT_SCALES = (0.125, 1.0)
GUARD = 4
BETAS, EPS = (0.9, 0.98), 1e-6


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(_bits(a), _bits(b)) if a.dtype == F32 else torch.equal(a.view(torch.int16), b.view(torch.int16))


def _rates(i):
    return 1e-3 * (1 + i % 3), 0.2 * (i % 2)


def _scale(i, lo, hi, mul):
    return 10.0 ** (lo + (hi - lo) * ((i * mul) % len(SIZES)) / (len(SIZES) - 1))


@pytest.fixture(scope="module")
def ragged(gpu_device):
    """Inputs of the kernel-level tests, left unchanged by them: gradients as views at odd 4-byte offsets of one flat buffer
    (randn times a per-tensor scale in [1e-3, 1e2]); weights (scale 1e-2 .. 1e1, one tensor all zeros), first moments and
    non-negative second moments of a run in progress.  -> (flat, [g], [w], [m], [v])."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    flat = torch.randn(sum(SIZES) + len(SIZES) + 1, device="cuda", generator=gen)
    gs, ws, ms, vs, o = [], [], [], [], 1
    for i, n in enumerate(SIZES):
        g = flat[o:o + n]
        g *= _scale(i, -3.0, 2.0, 7)
        gs.append(g)
        o += n + 1
        s = _scale(i, -3.0, 2.0, 7)
        ws.append(torch.randn(n, device="cuda", generator=gen) * (0.0 if i == ZERO else _scale(i, -2.0, 1.0, 3)))
        ms.append(torch.randn(n, device="cuda", generator=gen) * (0.3 * s))
        vs.append(torch.randn(n, device="cuda", generator=gen).square() * (0.02 * s * s))
    assert any(g.data_ptr() % 16 for g in gs) and any(g.data_ptr() % 16 == 0 for g in gs) and not bool(ws[ZERO].any())
    return flat, gs, ws, ms, vs


class State:
    """Owned copies of the weights and moments with NaN guard elements on both sides, and packed copies with guards."""

    def __init__(self, ragged, only=None):
        _, _, ws, ms, vs = ragged
        self.idx = list(range(len(SIZES))) if only is None else list(only)
        nan = float("nan")

        def guarded(t):
            buf = torch.full((t.numel() + 2 * GUARD,), nan, device="cuda")
            buf[GUARD:GUARD + t.numel()] = t
            return buf
        self.buf = {i: tuple(guarded(t[i]) for t in (ws, ms, vs)) for i in self.idx}
        self.pk = {i: torch.full((SIZES[i] + 2 * 8,), nan, dtype=dt, device="cuda") for i, (dt, _) in KINDS.items() if i in self.idx}
        if SPLIT in self.idx:
            self.pk[SPLIT] = torch.full((SIZES[SPLIT] + 2 * 8,), nan, dtype=BF, device="cuda")

    def view(self, i, j):
        return self.buf[i][j][GUARD:GUARD + SIZES[i]]

    def items(self, gs, rates=_rates):
        """-> (items, joined) as hip.AdamwPlan / hip.LambPlan take them; gs: this state's gradients, in self.idx order."""
        items, joined = [], []
        for i, g in zip(self.idx, gs):
            p, m, v = (self.view(i, j) for j in range(3))
            lr, wd = rates(i)
            pk = self.pk.get(i)
            if i == SPLIT:
                for k, (lo, hi) in enumerate(((0, SPLIT_AT), (SPLIT_AT, SIZES[i]))):
                    items.append((p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], lr, wd, pk[8 + lo:8 + hi], SPLIT_SCALES[k]))
                    joined.append(k == 1)
            else:
                items.append((p, g, m, v, lr, wd, None if pk is None else pk[8:8 + SIZES[i]], KINDS[i][1] if pk is not None else 1.0))
                joined.append(False)
        return items, joined

    def check_guards(self):
        for i in self.idx:
            for b in self.buf[i]:
                assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()), ("guard", SIZES[i])
        for i, pk in self.pk.items():
            assert bool(torch.isnan(pk[:8].float()).all()) and bool(torch.isnan(pk[-8:].float()).all()), ("packed guard", SIZES[i])

    def check_packs(self):
        for i, pk in self.pk.items():
            p, n = self.view(i, 0), SIZES[i]
            if i == SPLIT:
                want = torch.cat([(p[:SPLIT_AT] * SPLIT_SCALES[0]).to(BF), (p[SPLIT_AT:] * SPLIT_SCALES[1]).to(BF)])
            else:
                want = (p * KINDS[i][1]).to(pk.dtype)
            assert _same_bits(pk[8:8 + n], want), ("packed copy", n)


def _assert_same(a, b, what):
    for i in a.idx:
        for j, name in enumerate("pmv"):
            x, y = a.buf[i][j], b.buf[i][j]
            assert torch.equal(_bits(x), _bits(y)), (what, name, SIZES[i], (a.view(i, j) - b.view(i, j)).abs().max().item())
    for i in a.pk:
        assert torch.equal(a.pk[i].view(torch.int16) if a.pk[i].dtype == BF else _bits(a.pk[i]),
                           b.pk[i].view(torch.int16) if b.pk[i].dtype == BF else _bits(b.pk[i])), (what, "packed copy", SIZES[i])


def _poisoned(plan):
    """The plan's outputs start as NaN, with NaN guard elements behind them: every slot is written, nothing beyond is."""
    plan.lamb_partials = torch.full((2 * plan.n_chunks + 3,), float("nan"), device="cuda")
    plan.result = torch.full((3 * plan.n_params + 3,), float("nan"), device="cuda")
    flat = plan.result[:3 * plan.n_params].view(3, plan.n_params)
    plan.ratio, plan.param_norm, plan.update_norm = flat[0], flat[1], flat[2]
    return plan


def _outputs_intact(plan):
    torch.cuda.synchronize()
    assert bool(torch.isnan(plan.lamb_partials[2 * plan.n_chunks:]).all()) and bool(torch.isnan(plan.result[3 * plan.n_params:]).all())
    assert bool(torch.isfinite(plan.lamb_partials[:2 * plan.n_chunks]).all())


def _fp64_norms(ragged, step, coef=1.0):
    """Per parameter (||w||, ||u||, N) in fp64 from the device's own fp32 inputs."""
    _, gs, ws, ms, vs = ragged
    b1, b2 = np.float32(BETAS[0]).astype(np.float64), np.float32(BETAS[1]).astype(np.float64)      # the betas as the kernel receives them
    eps = float(np.float32(EPS))
    out = []
    for i in range(len(SIZES)):
        w, g, m, v = (t[i].double() for t in (ws, gs, ms, vs))
        g = (gs[i] * torch.tensor(coef, dtype=F32, device="cuda")).double() if coef != 1.0 else g   # ONE fp32 multiply, as the kernel's
        wd = float(np.float32(_rates(i)[1]))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        a = (m / (1 - b1 ** step)) / (torch.sqrt(v / (1 - b2 ** step)) + eps)
        u = a + wd * w
        out.append((float(torch.linalg.vector_norm(w)), float(torch.linalg.vector_norm(u)),
                    float(torch.linalg.vector_norm(a.abs() + (wd * w).abs()))))
    return out


# ---------------------------------------------------------------------------- 1. norms and ratios against fp64
def test_norms_and_ratios_against_fp64(ragged):
    _, gs, *_ = ragged
    st = State(ragged)
    items, joined = st.items(gs)
    assert sum((it[0].numel() + CHUNK - 1) // CHUNK for it in items) > 400 + 60 and len(items) > 2 * 32
    plan = _poisoned(hip.LambPlan(items, joined=joined))
    assert plan.n_params == len(SIZES) == plan.n - 1 and plan.arr[SPLIT].param == plan.arr[SPLIT + 1].param == SPLIT
    assert [plan.arr[i].adapt for i in range(4)] == [0, 1, 0, 1] and plan.arr[plan.n - 1].param == len(SIZES) - 1
    L, s = hip.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = [b.clone() for i in st.idx for b in st.buf[i]]

    def norms(trust_clip=0):
        assert L.msclip_lamb_partials(plan.arr, plan.n, *BETAS, EPS, 3, None, hip._p(plan.lamb_partials), 2 * plan.n_chunks, s) == 0
        assert L.msclip_lamb_ratios(hip._p(plan.lamb_partials), hip._p(plan.first_chunk), plan.n_params, plan.n_chunks, trust_clip,
                                    hip._p(plan.result), s) == 0
        _outputs_intact(plan)
        return plan.lamb_partials.clone(), plan.result.clone()
    partials, result = norms()
    # the two passes in front of the apply write nothing but their outputs
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, [b for i in st.idx for b in st.buf[i]]))
    plan.lamb_partials.fill_(float("nan"))
    plan.result.fill_(float("nan"))
    partials2, result2 = norms()
    assert torch.equal(_bits(partials), _bits(partials2)) and torch.equal(_bits(result), _bits(result2))      # bitwise repeatable
    r, wn, un = (t.tolist() for t in result[:3 * plan.n_params].view(3, -1))
    worst = {"w": 0.0, "u": 0.0, "r": 0.0}
    for i, (wn64, un64, N) in enumerate(_fp64_norms(ragged, 3)):
        if i == ZERO:
            assert wn[i] == 0.0 and r[i] == 1.0
            continue
        ew, eu = abs(wn[i] - wn64) / wn64, abs(un[i] - un64) / N
        worst["w"], worst["u"] = max(worst["w"], ew), max(worst["u"], eu)
        assert ew <= NORM_TOL and eu <= NORM_TOL, (SIZES[i], ew, eu)
        r64, e_u = wn64 / un64, NORM_TOL * N / un64
        er = abs(r[i] - r64) / r64
        worst["r"] = max(worst["r"], er / ((NORM_TOL + e_u) / (1 - e_u) + 2.0 ** -23))
        assert er <= (NORM_TOL + e_u) / (1 - e_u) + 2.0 ** -23, (SIZES[i], r[i], r64)
    print(f"worst ||w|| error {worst['w']:.3g} (bound {NORM_TOL:g}), worst ||u|| error / N {worst['u']:.3g} (bound {NORM_TOL:g}), "
          f"worst ratio error / its bound {worst['r']:.3g}")
    assert any(x > 1.0 for x in r) and any(0.0 < x < 1.0 for x in r)
    # 3. trust_clip: ratios above 1 become exactly 1.0, the others and the norms are untouched
    _, capped = norms(trust_clip=1)
    rc = capped[:plan.n_params]
    over = result[:plan.n_params] > 1.0
    assert bool((rc[over] == 1.0).all()) and torch.equal(_bits(rc[~over]), _bits(result[:plan.n_params][~over]))
    assert torch.equal(_bits(capped[plan.n_params:]), _bits(result[plan.n_params:]))


def test_ratio_is_exactly_one_where_nothing_adapts_or_a_norm_is_zero(ragged):
    _, gs, *_ = ragged
    n = 5000
    z = lambda: torch.zeros(n, device="cuda")                # noqa: E731
    w = torch.randn(n, device="cuda")
    w0 = w.clone()
    # u = 0: zero gradient and moments, wd = 0, always_adapt
    g0 = z()                                                 # (a plan does not keep its gradients alive)
    plan = _poisoned(hip.LambPlan([(w, g0, z(), z(), 1e-3, 0.0)], always_adapt=True))
    assert plan.arr[0].adapt == 1
    plan.run(*BETAS, EPS, 1)
    _outputs_intact(plan)
    assert plan.ratio[0].item() == 1.0 and plan.update_norm[0].item() == 0.0 and plan.param_norm[0].item() > 0 and torch.equal(w, w0)
    # non-adapting items take the plain Adam step whatever the norms are: r_eff = 1.0 exactly
    st, ref = State(ragged, only=range(12)), State(ragged, only=range(12))
    items, joined = st.items(gs[:12], rates=lambda i: (_rates(i)[0], 0.0))
    plan = hip.LambPlan(items, joined=joined)
    assert not any(plan.arr[i].adapt for i in range(plan.n))
    plan.run(*BETAS, EPS, 2)
    hip.AdamwPlan(*ref.items(gs[:12], rates=lambda i: (_rates(i)[0], 0.0))).run(*BETAS, EPS, 2)
    _assert_same(st, ref, "wd = 0 everywhere")
    assert bool((plan.ratio != 1.0).any())                   # (the ratios as computed are not 1: they were not used)
    # set_rates moves an item between the two kinds
    plan.set_rates([(1e-3, 0.1)] * plan.n)
    assert all(plan.arr[i].adapt for i in range(plan.n))


# ---------------------------------------------------------------------------- 2. the apply pass, bit for bit
@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
def test_apply_is_adamw_with_the_rate_scaled_by_the_device_ratio(ragged, clipped):
    flat, gs, *_ = ragged
    lamb, ref = State(ragged), State(ragged)
    items, joined = lamb.items(gs)
    plan = _poisoned(hip.LambPlan(items, joined=joined))
    ref_plan = hip.AdamwPlan(*ref.items(gs))
    item_tensor = [i for i in lamb.idx for _ in range(2 if i == SPLIT else 1)]
    n64 = float(torch.sqrt(sum(g.double().pow(2).sum() for g in gs)))
    for step in (1, 2):
        fs = flat * step                                               # this step's gradients: new addresses, same offsets
        ptrs = [fs[it[1].storage_offset():].data_ptr() for it in items]
        plan.set_grads(ptrs)
        ref_plan.set_grads(ptrs)
        max_norm = 0.5 * step * n64 if clipped else None
        plan.run(*BETAS, EPS, step, max_norm)
        _outputs_intact(plan)
        ratios = plan.ratio.cpu().numpy()                              # the device's own fp32 ratios
        rates = []
        for k, i in enumerate(item_tensor):
            lr, wd = _rates(i)
            assert plan.arr[k].param == i and plan.arr[k].adapt == int(wd != 0)
            rates.append((float(np.float32(lr) * ratios[i]) if wd else lr, wd))       # ONE fp32 multiply
        ref_plan.set_rates(rates)
        ref_plan.run(*BETAS, EPS, step, max_norm)
        if clipped:
            assert _same_bits(plan.clip, ref_plan.clip) and 0.49 < plan.coef.item() < 0.51
        _assert_same(lamb, ref, f"step {step}")
    assert rates[SPLIT] == rates[SPLIT + 1] and ratios[SPLIT] != 1.0                 # the split parameter: one ratio for both items
    lamb.check_guards()
    lamb.check_packs()
    _, _, ws, ms, vs = ragged
    assert not _same_bits(lamb.view(7, 0), ws[7]) and not _same_bits(lamb.view(8, 1), ms[8])
    assert torch.equal(fs, flat * 2)                                                 # no gradient was written


def test_clipped_update_norm_is_of_the_scaled_gradient(ragged):
    _, gs, *_ = ragged
    st = State(ragged)
    items, joined = st.items(gs)
    plan = _poisoned(hip.LambPlan(items, joined=joined))
    n64 = float(torch.sqrt(sum(g.double().pow(2).sum() for g in gs)))
    plan.run(*BETAS, EPS, 3, max_norm=0.25 * n64)
    _outputs_intact(plan)
    coef = plan.coef.item()
    assert abs(coef - 0.25) < 1e-4
    un = plan.update_norm.tolist()
    plain = _fp64_norms(ragged, 3)
    moved = 0
    for i, (_, un64, N) in enumerate(_fp64_norms(ragged, 3, coef=coef)):
        assert abs(un[i] - un64) <= NORM_TOL * N, (SIZES[i], un[i], un64)
        moved += abs(un64 - plain[i][1]) > 10 * NORM_TOL * N
    assert moved > len(SIZES) // 2                                      # (the unscaled gradient would have missed the bound)


# ---------------------------------------------------------------------------- 4. NaN / Inf
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_gradient_element(ragged, bad):
    _, gs, ws, ms, vs = ragged
    only, where = list(range(12)), 7                                    # tensor 7: odd index, wd = 0.2, it adapts; the split parameter
    clean, dirty = State(ragged, only=only), State(ragged, only=only)
    mine = [g.clone() for g in gs[:12]]
    at = SIZES[where] // 2 + 1
    mine[where][at] = bad
    hip.LambPlan(*clean.items(gs[:12])).run(*BETAS, EPS, 2)
    plan = hip.LambPlan(*dirty.items(mine))
    plan.run(*BETAS, EPS, 2)
    i = where
    lr, wd = _rates(i)
    ref = R.lamb_step({"x": ws[i].cpu()}, {"x": mine[i].cpu()}, {"x": (ms[i].cpu().double(), vs[i].cpu().double())}, 2, lr, wd,
                      betas=BETAS, eps=EPS)["x"]
    assert float(ref["raw"]) == 1.0                                     # the rule: a NaN norm fails both comparisons
    assert plan.ratio[i].item() == 1.0 and bool(torch.isnan(plan.update_norm[i]))
    got = dirty.view(i, 0)
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref["w"])) and int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got[at]))
    ok = torch.ones(SIZES[i], dtype=torch.bool)
    ok[at] = False
    delta = (got.cpu().double() - ref["w"])[ok].abs().max().item()
    assert delta <= 2.0 ** -23 * ws[i].abs().max().item() + 3e-5 * ref["delta"][ok].abs().max().item()
    for j in only:                                                      # the other tensors: finite, and bitwise the clean run's
        if j != where:
            for c in range(3):
                assert bool(torch.isfinite(dirty.view(j, c)).all()) and _same_bits(dirty.view(j, c), clean.view(j, c)), (SIZES[j], c)
    assert bool(torch.isfinite(plan.ratio[[j for j in only if j != where]]).all())
    dirty.check_guards()


# ---------------------------------------------------------------------------- 5-8. the training step
def _fresh():
    m = get_clip_model(named_config(B32, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(B32), strict=True)
    return m.cuda().eval()


def _data(seed, batch=4):
    return synth.synth_images(batch, seed=seed).cuda(), synth.synth_tokens(batch, seed=seed + 1).cuda()


@pytest.fixture(scope="module")
def b32_grads(gpu_device):
    """Two owned gradient dicts of the B/32 model at batch 4 (frozen statistics, the initial weights).  Every model below is
    built identically and stepped on THESE tensors, so bitwise comparisons hold (token_embedding.weight's atomic sums included)."""
    m = _fresh()
    ts = train.TrainStep(m, lr=1e-3, bn="frozen")
    out = []
    for seed in (51, 61):
        ts.forward(*_data(seed))
        out.append(ts.backward(clone=True))
    ts.saved = None
    assert len(out[0]) == 325 and "logit_scale" in out[0]
    return out


def _params64(m):
    return {k: p.detach().cpu().double() for k, p in m.named_parameters()}


def _state64(ts):
    return {k: (a.detach().cpu().double(), b.detach().cpu().double()) for k, (a, b) in ts.state.items()}


def _against_ref(m, ts, grads, before, state, step, what, coef=1.0, **kw):
    """The model's parameters after ts.step(grads) against lamb_ref on `before` / `state` (fp64 copies taken before the step)."""
    groups = {k: (lr, wd) for k, _, lr, wd in ts.param_groups()}
    assert sorted(grads) == sorted(before)                              # every parameter has a gradient
    ref = R.lamb_step(before, {k: g.detach().cpu() for k, g in grads.items()}, state, step, {k: v[0] for k, v in groups.items()},
                      {k: v[1] for k, v in groups.items()}, betas=ts.betas, eps=ts.eps, coef=coef, **kw)
    worst = (0.0, None)
    for k, p in m.named_parameters():
        o = ref[k]
        bound = 2.0 ** -23 * before[k].abs() + 3e-5 * o["delta"].abs().max()
        err = (p.detach().cpu().double() - o["w"]).abs()
        q = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, (q, k))
        assert q <= 1.0, (what, k, q, float(err.max()), float(o["delta"].abs().max()))
    print(f"{what}: worst |w - w_ref| / bound {worst[0]:.3g} ({worst[1]})")
    return ref


def _block_copies(eng):
    out = {}
    for blocks in ("tblk", "vblk"):
        for i, b in enumerate(getattr(eng, blocks)):
            if b is not None:
                for f in ("wqkv", "bqkv", "wo", "bo", "wfc", "bfc", "wpr", "bpr"):
                    out[f"{blocks}{i}.{f}"] = getattr(b["w"], f).clone()
    return out


def test_two_lamb_training_steps_against_the_reference(gpu_device):
    m = _fresh()
    ts = train.TrainStep(m, lr=1e-3, bn="frozen", optimizer="lamb")
    assert ts.eps == 1e-6 and ts.last_trust_ratio is None and train.TrainStep(m, lr=1e-3).eps == 1e-8
    names = [k for k, _ in m.named_parameters()]
    for step, seed in ((1, 51), (2, 61)):
        img, tok = _data(seed)
        ts.forward(img, tok)
        grads = ts.backward(clone=True)
        before, state = _params64(m), _state64(ts)
        ts.step(grads)
        ref = _against_ref(m, ts, grads, before, state, step, f"lamb step {step}")
        assert list(ts.last_trust_ratio) == names == list(ts.last_param_norm) == list(ts.last_update_norm)
        adapting = 0
        for k, _, _, wd in ts.param_groups():
            r, o = ts.last_trust_ratio[k], ref[k]
            assert r.dim() == 0 and r.is_cuda
            assert abs(ts.last_param_norm[k].item() - float(o["wn"])) <= NORM_TOL * float(o["wn"]), k
            if wd:
                adapting += 1
                assert abs(r.item() - float(o["r"])) <= 3e-5 * float(o["r"]), (k, r.item(), float(o["r"]))
        assert adapting > 50
    # in_proj_weight: two items of the table, one parameter, one ratio
    plan = ts._plan
    k = "visual.transformer.resblocks.3.attn.in_proj_weight"
    rows = [i for i, (name, _) in enumerate(plan.pieces) if name == k]
    assert len(rows) == 2 and plan.arr[rows[0]].param == plan.arr[rows[1]].param and plan.arr[rows[0]].adapt == 1
    assert plan.n_params == len(names) < plan.n
    # the engine's packed projection copies are casts of the new parameters, and the logits come from them
    got = _block_copies(ts.eng)
    loss = m.contrastive_loss(img, tok).item()
    ts.eng.refresh(force=True)                                          # the full pack from the module
    want = _block_copies(ts.eng)
    assert got.keys() == want.keys() and all(_same_bits(got[f], want[f]) for f in got), [f for f in got if not _same_bits(got[f], want[f])][:5]
    blk = m.visual.transformer.resblocks[3]
    assert torch.equal(ts.eng.vblk[3]["w"].wfc, blk.mlp.c_fc.weight.detach().to(BF))
    assert abs(loss - m.contrastive_loss(img, tok).item()) <= 2e-2


def test_lamb_composes_with_clipping_ema_and_the_schedule(b32_grads):
    g1, g2 = b32_grads
    N = float(torch.sqrt(sum(g.double().pow(2).sum() for g in g1.values())))
    m = _fresh()
    ts = train.TrainStep(m, lr=1e-3, bn="frozen", optimizer="lamb", clip_grad_norm=0.5 * N, ema_decay=0.9, trust_clip=True)
    before, state = _params64(m), _state64(ts)
    ts.step(g1)
    assert abs(ts.last_grad_norm.item() - N) <= NORM_TOL * N and abs(ts.last_clip_coef.item() - 0.5) < 1e-4
    ref = _against_ref(m, ts, g1, before, state, 1, "clipped lamb step, trust_clip", coef=ts.last_clip_coef.item(), trust_clip=True)
    assert max(t.item() for t in ts.last_trust_ratio.values()) <= 1.0 and len(ref) == 325
    # the shadow follows the LAMB-updated weights: decay * initial + (1 - decay) * new, three fp32 roundings
    assert ts.ema_updates == 1
    d, omd = hip.EmaPlan.coefficients(0.9)
    for k, p in m.named_parameters():
        want = d * before[k].float().cuda() + omd * p.detach()
        assert _same_bits(ts.ema_shadow[k], want), k
    # set_epoch changes only the rate: same table, same ratios, a step scaled by the schedule
    ma, mb = _fresh(), _fresh()
    ta = train.TrainStep(ma, lr=1e-3, bn="frozen", optimizer="lamb")
    tb = train.TrainStep(mb, lr=1e-3, bn="frozen", optimizer="lamb")
    tb.schedule = train.CosineSchedule(epochs=10, warmup_epochs=2, warmup_lr=1e-5)
    ta.step(g1)
    tb.step(g1)
    plan = tb._plan
    tb.set_epoch(1)                                                     # warm-up: (1e-5 + 1e-3) / 2
    assert abs(tb.lr - 0.505e-3) < 1e-12
    before, state = _params64(mb), _state64(tb)
    ta.step(g2)
    tb.step(g2)
    assert tb._plan is plan and plan.rates_for[0] == tb.lr
    for k in ta.last_trust_ratio:
        assert _same_bits(ta.last_trust_ratio[k], tb.last_trust_ratio[k]) and _same_bits(ta.last_update_norm[k], tb.last_update_norm[k]), k
    _against_ref(mb, tb, g2, before, state, 2, "lamb step at the scheduled rate")
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert not _same_bits(pa["visual.proj"].data, pb["visual.proj"].data)


def test_lamb_after_accumulate(gpu_device):
    """accumulate() hands step() the gradient SUMMED over the chunks, as it does under AdamW: the LAMB step on it is the step
    lamb_ref takes on that sum, and bitwise the step of a second TrainStep handed owned copies of it.  Against the one-shot
    forward / backward / step on the whole batch the UPDATES agree within the block bound that the accumulate tests put on
    gradients (tests/gradcheck.py: WORST_MARGIN on every 64-row / 64-column block, the embedding table by its touched rows)."""
    img, tok = _data(0, batch=8)
    ma, mb, mc = _fresh(), _fresh(), _fresh()
    ta = train.TrainStep(ma, lr=1e-3, bn="frozen", optimizer="lamb")
    tb = train.TrainStep(mb, lr=1e-3, bn="frozen", optimizer="lamb")
    tc = train.TrainStep(mc, lr=1e-3, bn="frozen", optimizer="lamb")
    start = {k: p.detach().clone() for k, p in ma.named_parameters()}
    _, grads = ta.accumulate([(img[:4], tok[:4]), (img[4:], tok[4:])])
    owned = {k: g.clone() for k, g in grads.items()}
    before, state = _params64(ma), _state64(ta)
    ta.step(grads)
    _against_ref(ma, ta, owned, before, state, 1, "lamb step after accumulate(2 chunks)")
    tb.step(owned)
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert all(_same_bits(pa[k].data, pb[k].data) for k in pa)
    tc.forward(img, tok)
    tc.step(tc.backward())
    worst = (0.0, None)
    for k, p in mc.named_parameters():
        got, want = pa[k].data - start[k], p.data - start[k]
        fig = G.measure_one(k, got, want)
        worst = max(worst, (fig["block"], k))
        if k == TOK:
            assert fig["stray_rows"] == 0 and fig["row_err"] <= G.WORST_MARGIN, fig
        else:
            assert fig["block"] <= G.WORST_MARGIN, (k, fig)
    print(f"update after accumulate(2 chunks) against the one-shot step's: worst block error {worst[0]:.3g} ({worst[1]})")


def test_lamb_checkpoint_round_trip(b32_grads, tmp_path):
    g1, g2 = b32_grads
    ma = _fresh()
    ta = train.TrainStep(ma, lr=1e-3, bn="frozen", optimizer="lamb", trust_clip=True)
    ta.step(g1)
    path = tmp_path / "lamb.pth"
    train.save_checkpoint(ma, ta, path, step=0, model_name=B32)
    obj = torch.load(path, weights_only=False)
    assert set(obj) == {"step", "model", "state_dict", "perf", "optimizer"}
    assert obj["optimizer"]["msclip"]["optimizer"] == "lamb" and obj["optimizer"]["param_groups"][0]["trust_clip"] is True
    assert obj["optimizer"]["param_groups"][0]["eps"] == 1e-6 and "amsgrad" not in obj["optimizer"]["param_groups"][0]
    ta.step(g2)
    mb = _fresh()
    tb = train.TrainStep(mb, lr=1e-3, bn="frozen", optimizer="lamb", trust_clip=True)
    assert train.resume_checkpoint(mb, tb, path) == 1 and tb.steps == 1
    tb.step(g2)
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert all(_same_bits(pa[k].data, pb[k].data) for k in pa)
    assert all(_same_bits(ta.state[k][j], tb.state[k][j]) for k in ta.state for j in (0, 1))
    assert all(_same_bits(ta.last_trust_ratio[k], tb.last_trust_ratio[k]) for k in ta.last_trust_ratio)
    # the other optimizer refuses the file, before it loads anything
    mc = _fresh()
    tc = train.TrainStep(mc, lr=1e-3, bn="frozen")
    with pytest.raises(ValueError, match="lamb"):
        train.resume_checkpoint(mc, tc, path)
    assert tc.steps == 0 and not tc.state
    # and an adamW checkpoint carries no trace of the new keys
    tc.step(g1)
    train.save_checkpoint(mc, tc, tmp_path / "adamw.pth", step=0, model_name=B32)
    opt = torch.load(tmp_path / "adamw.pth", weights_only=False)["optimizer"]
    assert set(opt["msclip"]) == {"steps", "bn", "names"} and set(opt["param_groups"][0]) == {"lr", "weight_decay", "betas", "eps", "amsgrad", "params"}
    with pytest.raises(ValueError, match="adamw"):
        train.resume_checkpoint(ma, ta, tmp_path / "adamw.pth")


# ---------------------------------------------------------------------------- 8. adamW is what it was
def test_adamw_argument_is_the_default_step(b32_grads, monkeypatch):
    """Needs the parent's behaviour only: optimizer="adamw" is the default TrainStep, bit for bit, and its step() makes the
    optimizer calls it made before lamb existed -- one msclip_adamw_multi, none of the LAMB entry points."""
    g1, g2 = b32_grads
    ma, mb = _fresh(), _fresh()
    ta = train.TrainStep(ma, lr=1e-4, bn="frozen")
    tb = train.TrainStep(mb, lr=1e-4, bn="frozen", optimizer="adamW")
    L = hip.lib()
    calls = []
    watched = ("msclip_adamw_multi", "msclip_adamw_multi_clipped", "msclip_adamw", "msclip_grad_sumsq", "msclip_clip_coef",
               "msclip_ema_multi") + tuple(n for n in hip.EXT3_EXPORTS if n != "msclip_ext3_abi_version")
    for name in watched:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    for g in (g1, g2):
        ta.step(g)
        tb.step(g)
    assert calls == ["msclip_adamw_multi"] * 4
    assert type(tb._plan) is hip.AdamwPlan and tb.last_trust_ratio is None and tb.last_param_norm is None and tb.last_update_norm is None
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert all(_same_bits(pa[k].data, pb[k].data) for k in pa)
    assert all(_same_bits(ta.state[k][j], tb.state[k][j]) for k in ta.state for j in (0, 1))
    del calls[:]
    tl = train.TrainStep(_fresh(), lr=1e-3, bn="frozen", optimizer="lamb", clip_grad_norm=1.0, ema_decay=0.5)
    tl.step(g1)
    assert calls == ["msclip_grad_sumsq", "msclip_clip_coef", "msclip_lamb_partials", "msclip_lamb_ratios", "msclip_lamb_apply",
                     "msclip_ema_multi"]
    with pytest.raises(NotImplementedError):
        train.TrainStep(ma, lr=1e-4, optimizer="sgd")
