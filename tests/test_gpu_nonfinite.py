"""The non-finite guard of the optimizer phase on a real MI355X (include/msclip_ext4.h, TrainStep(nonfinite=...)): the verdict
kernel against msclip_clip_coef and tests/nonfinite_ref.py, the guarded updates bit for bit against the unguarded ones and
writing nothing on a skip, and TrainStep beside unguarded twins: a run with skipped steps ends where the run without those steps
ends, bit for bit.  Everything here is an equality of bits or of integers: no tolerance is used.

The non-finite values are ordinary NaN / Inf numbers written into partials or gradient tensors.  The training-step tests run
step() on precomputed gradient dicts of the ViT-B/32 model at batch 8 (frozen BatchNorm, no stochastic depth), so that twins are
stepped on the same bits (token_embedding.weight's atomic sums included)."""
import ctypes

import pytest
import torch

import nonfinite_ref as R
from conftest import synth_sd
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
B32 = "b32-yfcc-msclips"
NAN, INF = float("nan"), float("inf")
BETAS, EPS = (0.9, 0.98), 1e-6
SENT_I = 0x5A5A5A5A
PAD = 4


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(I32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------- 1. the verdict
class Verdict:
    """partials, out and state as the inner parts of padded buffers: sentinel words on both sides of each."""

    def __init__(self, partials, total=0):
        n = partials.numel()
        self.n = n
        self.pbuf = torch.full((n + 2 * PAD,), 123.0, device="cuda")
        self.pbuf[PAD:PAD + n] = partials
        self.partials = self.pbuf[PAD:PAD + n]
        self.obuf = torch.full((2 + 2 * PAD,), -7.0, device="cuda")
        self.out = self.obuf[PAD:PAD + 2]
        self.sbuf = torch.full((4 + 2 * PAD,), SENT_I, dtype=I32, device="cuda")
        self.state = self.sbuf[PAD:PAD + 4]
        self.state.copy_(torch.tensor([9, total, 9, 9], dtype=I32))

    def run(self, max_norm):
        assert hip.lib().msclip_clip_coef_guarded(hip._p(self.partials), self.n, float(max_norm), hip._p(self.out), hip._p(self.state),
                                                  _stream()) == 0
        torch.cuda.synchronize()
        assert bool((self.obuf[:PAD] == -7.0).all()) and bool((self.obuf[PAD + 2:] == -7.0).all()), "words around out"
        assert bool((self.sbuf[:PAD] == SENT_I).all()) and bool((self.sbuf[PAD + 4:] == SENT_I).all()), "words around state"
        assert bool((self.pbuf[:PAD] == 123.0).all()) and bool((self.pbuf[PAD + self.n:] == 123.0).all())
        return self.out.clone(), self.state.tolist()


def _plain(partials, max_norm):
    out = torch.full((2,), -7.0, device="cuda")
    assert hip.lib().msclip_clip_coef(hip._p(partials), partials.numel(), float(max_norm), hip._p(out), _stream()) == 0
    torch.cuda.synchronize()
    return out


def _partials(n):
    gen = torch.Generator(device="cuda").manual_seed(n)
    return torch.rand(n, device="cuda", generator=gen) * 10.0 + 1e-3


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 4292])
def test_verdict_on_finite_partials_is_clip_coef(gpu_device, n):
    part = _partials(n)
    norm = R.norm64(part.cpu())
    v = Verdict(part, total=5)
    for max_norm in (0.0, 0.5 * norm, 2.0 * norm):
        out, state = v.run(max_norm)
        assert _same_bits(out, _plain(v.partials, max_norm)), (n, max_norm)
        assert state == [0, 5, -1, 0] == R.verdict(part.cpu(), 5)
        again, state2 = v.run(max_norm)                                 # bitwise repeatable
        assert _same_bits(out, again) and state2 == state
    assert abs(out[0].item() - norm) <= 1e-5 * norm and out[1].item() == 1.0


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 4292])
@pytest.mark.parametrize("bad", [NAN, INF, -INF], ids=["nan", "inf", "-inf"])
def test_verdict_on_a_non_finite_partial(gpu_device, n, bad):
    part = _partials(n)
    total = 0
    v = Verdict(part)
    for at in sorted({0, n - 1, 255, 256}):
        if at >= n:
            continue
        keep = v.partials[at].clone()
        v.partials[at] = bad
        out, state = v.run(1.0)
        total += 1
        assert state == [1, total, at, 1] == R.verdict(v.partials.cpu(), total - 1), (n, at)
        assert not bool(torch.isfinite(out[0]))
        assert _same_bits(out, _plain(v.partials, 1.0))
        v.partials[at] = keep
    out, state = v.run(1.0)                                              # clean again: the verdict clears, the total stays
    assert state == [0, total, -1, 0] and bool(torch.isfinite(out).all())


def test_verdict_reports_the_smaller_index_and_accumulates(gpu_device):
    part = _partials(1023)
    v = Verdict(part, total=0)
    for k, (a, b) in enumerate(((700, 3), (3, 700), (256, 255), (1022, 0), (511, 512)), 1):
        keep = v.partials.clone()
        v.partials[a], v.partials[b] = NAN, -INF
        _, state = v.run(0.0)
        assert state == [1, k, min(a, b), 2] == R.verdict(v.partials.cpu(), k - 1)
        v.partials.copy_(keep)
    _, state = v.run(0.0)
    assert state == [0, 5, -1, 0]                                        # five calls, five skips counted
    v.partials.fill_(INF)
    _, state = v.run(0.0)
    assert state == [1, 6, 0, 1023]


# ---------------------------------------------------------------------------- 2, 3. the guarded updates
SIZES = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 32767, 32768, 32769, 65535, 65536, 65537,
         65541, 9, 33, 100, 1000, 5000, 12345, 33333, 40000, 50001, 6, 10, 12, 65540]
GUARD = 8


def _rates(i):
    return 1e-3 * (1 + i % 3), 0.2 * (i % 2)


def _offsets(shift):
    """Element offsets of the 40 tensors in an arena: tensor i starts (i + shift) % 4 elements behind a 16-byte boundary, with
    at least GUARD guard elements in front of it.  -> (offsets, arena length)."""
    offs, cur = [], GUARD
    for i, n in enumerate(SIZES):
        cur += (((i + shift) % 4) - cur) % 4
        offs.append(cur)
        cur += n + GUARD
    return offs, cur + GUARD


class Arena:
    """p, m, v and the packed copies of the 40 tensors, NaN guard words between them; `g` arenas are built by _grads."""

    def __init__(self, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.offs, total = _offsets(0)
        self.p, self.m, self.v = (torch.full((total,), NAN, device="cuda") for _ in range(3))
        self.pkb = torch.full((total,), NAN, dtype=BF, device="cuda")
        self.pkf = torch.full((total,), NAN, device="cuda")
        for i, (o, n) in enumerate(zip(self.offs, SIZES)):
            self.p[o:o + n] = torch.randn(n, device="cuda", generator=gen)
            self.m[o:o + n] = torch.randn(n, device="cuda", generator=gen) * 0.1
            self.v[o:o + n] = torch.randn(n, device="cuda", generator=gen).square() * 0.01
        self.all = (self.p, self.m, self.v, self.pkb, self.pkf)

    def items(self, g):
        out = []
        for i, (o, n) in enumerate(zip(self.offs, SIZES)):
            lr, wd = _rates(i)
            pk = (None, self.pkb, self.pkf)[i % 3]
            out.append((self.p[o:o + n], g[1][g[0][i]:g[0][i] + n], self.m[o:o + n], self.v[o:o + n], lr, wd,
                        None if pk is None else pk[o:o + n], 0.125 if i % 2 else 1.0))
        return out

    def snapshot(self):
        return [t.clone() for t in self.all]

    def same_as(self, other):
        """Every byte of every buffer, guard words included."""
        other = other.all if isinstance(other, Arena) else other
        return all(_same_bits(a, b) for a, b in zip(self.all, other))


def _grads(seed, shift, scale=1.0, poison=False):
    """Gradients in an arena of their own, at alignments shifted against the parameters' for half of the tensors (so that some
    tensors at a 16-byte parameter offset still take the 4-byte path).  -> (offsets, arena)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    offs, total = _offsets(0)
    if shift:
        offs = [o + (1 if i % 8 == 4 else 0) for i, o in enumerate(offs)]
    g = torch.full((total + 1,), NAN, device="cuda")
    for i, (o, n) in enumerate(zip(offs, SIZES)):
        g[o:o + n] = torch.randn(n, device="cuda", generator=gen) * (0.1 * scale)
        if poison and i % 7 == 3:
            g[o + n // 2] = NAN if i % 2 else INF
    return offs, g


@pytest.fixture(scope="module")
def update_grads(gpu_device):
    """Two steps' gradients and a poisoned set, shared and left unchanged."""
    return _grads(100, True), _grads(101, True, scale=2.0), _grads(102, True, poison=True)


def _skip_flag(value):
    return torch.tensor([value, 0, -1, 0], dtype=I32, device="cuda")


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
def test_guarded_adamw(update_grads, clipped):
    g1, g2, gbad = update_grads
    L, s = hip.lib(), _stream()
    mine, twin = Arena(7), Arena(7)
    assert mine.same_as(twin)
    clip = torch.tensor([3.0, 0.37], device="cuda")
    coef = ctypes.c_void_p(clip.data_ptr() + 4) if clipped else None
    go = _skip_flag(0)
    paths = set()
    for step, g in ((1, g1), (2, g2)):
        pa, pb = hip.AdamwPlan(mine.items(g)), hip.AdamwPlan(twin.items(g))
        assert pa.n == 40 > 36                                           # two launches: the table holds 36 items
        for i in range(pa.n):
            a = pa.arr[i]
            paths.add(not ((a.p | a.g | a.m | a.v) & 15) and not ((a.pk or 0) & (15 if a.pk_f32 else 7)))
        assert L.msclip_adamw_multi_guarded(pa.arr, pa.n, *BETAS, EPS, step, coef, hip._p(go), s) == 0
        if clipped:
            assert L.msclip_adamw_multi_clipped(pb.arr, pb.n, *BETAS, EPS, step, coef, s) == 0
        else:
            assert L.msclip_adamw_multi(pb.arr, pb.n, *BETAS, EPS, step, s) == 0
        torch.cuda.synchronize()
        assert mine.same_as(twin), f"step {step}"
    assert paths == {True, False}                                        # both access paths were taken
    assert not mine.same_as(Arena(7)) and go.tolist() == [0, 0, -1, 0]
    o, n = mine.offs[26], SIZES[26]                                      # 65 541 elements: three chunks, fp32 packed copy
    assert _same_bits(mine.pkf[o:o + n], mine.p[o:o + n] * 1.0) and bool(torch.isnan(mine.pkf[o - GUARD:o]).all())
    # skip = 1 with NaN and Inf in the gradients: every byte of every buffer stays, in both launches
    before = mine.snapshot()
    stop = _skip_flag(1)
    pa = hip.AdamwPlan(mine.items(gbad))
    assert L.msclip_adamw_multi_guarded(pa.arr, pa.n, *BETAS, EPS, 3, coef, hip._p(stop), s) == 0
    torch.cuda.synchronize()
    assert mine.same_as(before) and stop.tolist() == [1, 0, -1, 0]
    # ... which the unguarded call on the same gradients does not do
    assert L.msclip_adamw_multi(pa.arr, pa.n, *BETAS, EPS, 3, s) == 0
    torch.cuda.synchronize()
    assert not mine.same_as(before) and bool(torch.isnan(mine.p[mine.offs[3]:mine.offs[3] + SIZES[3]]).any())


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
def test_guarded_lamb_apply(update_grads, clipped):
    g1, g2, gbad = update_grads
    L, s = hip.lib(), _stream()
    mine, twin = Arena(9), Arena(9)
    clip = torch.tensor([3.0, 0.37], device="cuda")
    coef = ctypes.c_void_p(clip.data_ptr() + 4) if clipped else None
    ratio = torch.rand(40, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) + 0.5
    go = _skip_flag(0)
    for step, g in ((1, g1), (2, g2)):
        pa, pb = hip.LambPlan(mine.items(g)), hip.LambPlan(twin.items(g))
        assert pa.n == 40 > 32 and pa.n_params == 40 and sum(pa.arr[i].adapt for i in range(40)) == 20
        assert L.msclip_lamb_apply_guarded(pa.arr, pa.n, *BETAS, EPS, step, coef, hip._p(ratio), hip._p(go), s) == 0
        assert L.msclip_lamb_apply(pb.arr, pb.n, *BETAS, EPS, step, coef, hip._p(ratio), s) == 0
        torch.cuda.synchronize()
        assert mine.same_as(twin), f"step {step}"
    assert not mine.same_as(Arena(9))
    before = mine.snapshot()
    stop = _skip_flag(1)
    pa = hip.LambPlan(mine.items(gbad))
    assert L.msclip_lamb_apply_guarded(pa.arr, pa.n, *BETAS, EPS, 3, coef, hip._p(ratio), hip._p(stop), s) == 0
    torch.cuda.synchronize()
    assert mine.same_as(before) and stop.tolist() == [1, 0, -1, 0]


# ---------------------------------------------------------------------------- 4-8. the training step
def _fresh():
    m = get_clip_model(named_config(B32, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(B32), strict=True)
    return m.cuda().eval()


def _data(seed, batch=8):
    return synth.synth_images(batch, seed=seed).cuda(), synth.synth_tokens(batch, seed=seed + 1).cuda()


@pytest.fixture(scope="module")
def b32_grads(gpu_device):
    """Two owned gradient dicts of the B/32 model at batch 8 (frozen statistics, the initial weights), left unchanged."""
    m = _fresh()
    ts = train.TrainStep(m, lr=1e-3, bn="frozen")
    out = []
    for seed in (51, 61):
        ts.forward(*_data(seed))
        out.append(ts.backward(clone=True))
    ts.saved = None
    assert len(out[0]) == 325 and all(bool(torch.isfinite(g).all()) for d in out for g in d.values())
    return out


POISON_KEY = "visual.transformer.resblocks.3.attn.in_proj_weight"      # two items of the table, one entry of the norm's
OTHER_KEY = "token_embedding.weight"                                     # many chunks


def _poisoned(grads, key=POISON_KEY, value=NAN, at=None):
    out = dict(grads)
    g = grads[key].clone()
    g.view(-1)[g.numel() - 5 if at is None else at] = value
    out[key] = g
    return out


def _block_copies(eng):
    out = {}
    for blocks in ("tblk", "vblk"):
        for i, b in enumerate(getattr(eng, blocks)):
            if b is not None:
                for f in ("wqkv", "bqkv", "wo", "bo", "wfc", "bfc", "wpr", "bpr"):
                    out[f"{blocks}{i}.{f}"] = getattr(b["w"], f)
    return out


def _assert_twins(ma, ta, mb, tb, what, logits=True):
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    diff = [k for k in pa if not _same_bits(pa[k].data, pb[k].data)]
    assert not diff, (what, "parameters", diff[:5])
    assert ta.state.keys() == tb.state.keys()
    diff = [k for k in ta.state for j in (0, 1) if not _same_bits(ta.state[k][j], tb.state[k][j])]
    assert not diff, (what, "moments", diff[:5])
    ca, cb = _block_copies(ta.eng), _block_copies(tb.eng)
    diff = [f for f in ca if not _same_bits(ca[f], cb[f])]
    assert ca.keys() == cb.keys() and not diff, (what, "packed copies", diff[:5])
    if logits:
        img, tok = _data(7)
        with torch.no_grad():
            assert _same_bits(ma(img, tok).float(), mb(img, tok).float()), (what, "logits")


def _pair(**kw):
    ma, mb = _fresh(), _fresh()
    return ma, train.TrainStep(ma, lr=1e-3, bn="frozen", nonfinite="skip", **kw), mb, train.TrainStep(mb, lr=1e-3, bn="frozen", **kw)


def test_guarded_run_without_skips_is_the_unguarded_run(b32_grads):
    g1, g2 = b32_grads
    ma, ta, mb, tb = _pair()
    assert ta.last_skipped is None and ta.skipped_steps == 0 and tb.nonfinite is None
    for g in (g1, g2, g1):
        ta.step(g)
        tb.step(g)
        assert ta.last_skipped.dim() == 0 and ta.last_skipped.is_cuda and ta.last_skipped.dtype == I32
    _assert_twins(ma, ta, mb, tb, "three clean steps")
    assert ta.skipped_steps == 0 and ta.applied_steps == 3 == ta.steps and int(ta.last_skipped) == 0
    assert ta.nonfinite_gradients() == []
    # guarding without clipping: the norm is there, the coefficient is not
    want = hip.grad_norm([g1[k].contiguous().view(-1) for k, _ in ma.named_parameters()])
    assert _same_bits(ta.last_grad_norm, want) and ta.last_clip_coef is None
    assert tb.last_grad_norm is None and tb.last_skipped is None and tb.skipped_steps == 0
    with pytest.raises(ValueError):
        train.TrainStep(mb, lr=1e-3, nonfinite="ignore")
    with pytest.raises(RuntimeError):
        tb.nonfinite_gradients()


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
def test_a_skipped_step_leaves_no_trace(b32_grads, value):
    g1, g2 = b32_grads
    ma, ta, mb, tb = _pair()
    ta.step(g1)
    tb.step(g1)
    before = {k: p.detach().clone() for k, p in ma.named_parameters()}
    ta.step(_poisoned(g2, value=value))
    assert ta.nonfinite_gradients() == [POISON_KEY]                      # read right after the poisoned step
    assert int(ta.last_skipped) == 1 and not bool(torch.isfinite(ta.last_grad_norm))
    assert all(_same_bits(p.data, before[k]) for k, p in ma.named_parameters())
    for g in (g2, g1):
        ta.step(g)
    for g in (g2, g1):
        tb.step(g)
    _assert_twins(ma, ta, mb, tb, "g1, poisoned g2, g2, g1 beside g1, g2, g1")
    assert (ta.steps, ta.applied_steps, ta.skipped_steps) == (4, 3, 1) and tb.steps == 3
    assert int(ta.last_skipped) == 0 and ta.nonfinite_gradients() == []


def test_poison_in_the_very_first_step(b32_grads):
    g1, g2 = b32_grads
    ma, ta, mb, tb = _pair()
    ta.step(_poisoned(_poisoned(g1, key=OTHER_KEY, value=-INF, at=40000), value=NAN))
    assert ta.nonfinite_gradients() == [k for k, _ in ma.named_parameters() if k in (OTHER_KEY, POISON_KEY)]      # the table's order
    assert ta.skipped_steps == 1 and ta.applied_steps == 0
    assert all(bool((m == 0).all()) and bool((v == 0).all()) for m, v in ta.state.values())
    for g in (g1, g2):
        ta.step(g)
        tb.step(g)
    _assert_twins(ma, ta, mb, tb, "poisoned g1, g1, g2 beside g1, g2")
    assert (ta.steps, ta.applied_steps, ta.skipped_steps) == (3, 2, 1)


# ---------------------------------------------------------------------------- 5. composition
def test_skip_composes_with_clipping(b32_grads):
    g1, g2 = b32_grads
    N = float(torch.sqrt(sum(g.double().pow(2).sum() for g in g1.values())))
    ma, ta, mb, tb = _pair(clip_grad_norm=0.5 * N)
    ta.step(_poisoned(g1))
    assert bool(torch.isnan(ta.last_clip_coef)) and int(ta.last_skipped) == 1
    for g in (g1, g2):
        ta.step(g)
        tb.step(g)
        assert _same_bits(ta.last_grad_norm, tb.last_grad_norm) and _same_bits(ta.last_clip_coef, tb.last_clip_coef)
    assert 0.0 < tb.last_clip_coef.item() <= 1.0
    _assert_twins(ma, ta, mb, tb, "clipped", logits=False)
    assert ta.applied_steps == 2 and ta.skipped_steps == 1


def test_skip_composes_with_lamb(b32_grads):
    g1, g2 = b32_grads
    ma, ta, mb, tb = _pair(optimizer="lamb", clip_grad_norm=1.0)
    ta.step(_poisoned(g1, value=INF))
    assert ta.nonfinite_gradients() == [POISON_KEY]
    for g in (g1, g2):
        ta.step(g)
        tb.step(g)
        assert all(_same_bits(ta.last_trust_ratio[k], tb.last_trust_ratio[k]) for k in tb.last_trust_ratio)
    _assert_twins(ma, ta, mb, tb, "lamb", logits=False)
    assert type(ta._plan) is hip.LambPlan and ta.applied_steps == 2 and ta.skipped_steps == 1


def test_skip_composes_with_ema(b32_grads):
    """On the skipped step the shadows take one more pull toward the unchanged parameters: torch's three-operation formula."""
    g1, g2 = b32_grads
    ma, ta, mb, tb = _pair(ema_decay=0.9)
    d, omd = hip.EmaPlan.coefficients(0.9)
    shadow = {k: p.detach().clone() for k, p in ma.named_parameters()}
    for g in (_poisoned(g1), g1, g2):
        ta.step(g)
        shadow = {k: d * shadow[k] + omd * p.detach() for k, p in ma.named_parameters()}
    for g in (g1, g2):
        tb.step(g)
    assert ta.ema_updates == 3 and tb.ema_updates == 2
    assert all(_same_bits(ta.ema_shadow[k], shadow[k]) for k in shadow)
    assert not all(_same_bits(ta.ema_shadow[k], tb.ema_shadow[k]) for k in shadow)     # (one update more than the twin's)
    _assert_twins(ma, ta, mb, tb, "ema", logits=False)


def test_skip_after_accumulate(gpu_device):
    """The verdict is on the sum over the chunks: a NaN in the accumulators skips the step that follows accumulate()."""
    img, tok = _data(0)
    chunks = [(img[:4], tok[:4]), (img[4:], tok[4:])]
    ma, ta, mb, tb = _pair()
    _, grads = ta.accumulate(chunks)
    owned = {k: g.clone() for k, g in grads.items()}
    grads[POISON_KEY].view(-1)[17] = NAN                                 # into the accumulator itself
    ta.step(grads)
    assert ta.nonfinite_gradients() == [POISON_KEY] and ta.skipped_steps == 1
    _, grads = ta.accumulate(chunks)
    for k, g in grads.items():                                           # the twin's bits (the embedding table's sums are atomic)
        g.copy_(owned[k])
    ta.step(grads)
    tb.step(owned)
    _assert_twins(ma, ta, mb, tb, "accumulate", logits=False)
    assert (ta.steps, ta.applied_steps) == (2, 1)


# ---------------------------------------------------------------------------- 6. raise
def test_raise_names_the_tensor_and_keeps_the_state(b32_grads):
    g1, g2 = b32_grads
    ma, mb = _fresh(), _fresh()
    ta = train.TrainStep(ma, lr=1e-3, bn="frozen", nonfinite="raise")
    tb = train.TrainStep(mb, lr=1e-3, bn="frozen")
    ta.step(g1)
    tb.step(g1)
    params = {k: p.detach().clone() for k, p in ma.named_parameters()}
    moments = {k: (m.clone(), v.clone()) for k, (m, v) in ta.state.items()}
    with pytest.raises(FloatingPointError, match=POISON_KEY.replace(".", r"\.")):
        ta.step(_poisoned(g2))
    assert all(_same_bits(p.data, params[k]) for k, p in ma.named_parameters())
    assert all(_same_bits(ta.state[k][j], moments[k][j]) for k in moments for j in (0, 1))
    assert ta.skipped_steps == 1 and ta.nonfinite_gradients() == [POISON_KEY]
    ta.step(g2)                                                          # the next clean step applies
    tb.step(g2)
    _assert_twins(ma, ta, mb, tb, "raise", logits=False)
    assert (ta.steps, ta.applied_steps, ta.skipped_steps) == (3, 2, 1)


# ---------------------------------------------------------------------------- 7. checkpoint
def test_checkpoint_round_trip_after_a_skip(b32_grads, tmp_path):
    g1, g2 = b32_grads
    ma = _fresh()
    ta = train.TrainStep(ma, lr=1e-3, bn="frozen", nonfinite="skip")
    ta.step(g1)
    ta.step(_poisoned(g2))
    path = tmp_path / "guard.pth"
    train.save_checkpoint(ma, ta, path, step=1, model_name=B32)
    opt = torch.load(path, weights_only=False)["optimizer"]
    assert set(opt["msclip"]) == {"steps", "bn", "names", "skipped_steps"}
    assert opt["msclip"]["steps"] == 2 and opt["msclip"]["skipped_steps"] == 1
    assert {float(st["step"]) for st in opt["state"].values()} == {1.0}
    ta.step(g2)
    ta.step(g1)
    # resumed with the guard: both counters return, the run stays bitwise with the uninterrupted one
    mb = _fresh()
    tb = train.TrainStep(mb, lr=1e-3, bn="frozen", nonfinite="skip")
    assert train.resume_checkpoint(mb, tb, path) == 2
    assert (tb.steps, tb.skipped_steps, tb.applied_steps) == (2, 1, 1)
    tb.step(g2)
    tb.step(g1)
    _assert_twins(ma, ta, mb, tb, "resumed with the guard", logits=False)
    assert (tb.steps, tb.skipped_steps) == (4, 1)
    # resumed WITHOUT the guard: steps is the applied count
    mc = _fresh()
    tc = train.TrainStep(mc, lr=1e-3, bn="frozen")
    train.resume_checkpoint(mc, tc, path)
    assert tc.steps == 1 and tc.skipped_steps == 0
    tc.step(g2)
    tc.step(g1)
    _assert_twins(ma, ta, mc, tc, "resumed without the guard", logits=False)
    # and an unguarded checkpoint carries no trace of the feature
    train.save_checkpoint(mc, tc, tmp_path / "plain.pth", step=3, model_name=B32)
    opt = torch.load(tmp_path / "plain.pth", weights_only=False)["optimizer"]
    assert set(opt["msclip"]) == {"steps", "bn", "names"} and opt["msclip"]["steps"] == 3


# ---------------------------------------------------------------------------- 8. the off path
def test_entry_points_called_with_the_guard_off_and_on(b32_grads, monkeypatch):
    g1, g2 = b32_grads
    L = hip.lib()
    calls = []
    ext4 = tuple(n for n in hip.EXT4_EXPORTS if n != "msclip_ext4_abi_version")
    watched = ("msclip_adamw_multi", "msclip_adamw_multi_clipped", "msclip_adamw", "msclip_grad_sumsq", "msclip_clip_coef",
               "msclip_ema_multi") + tuple(n for n in hip.EXT3_EXPORTS if n != "msclip_ext3_abi_version") + ext4
    for name in watched:
        real = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    t0 = train.TrainStep(_fresh(), lr=1e-3, bn="frozen")
    assert t0.nonfinite is None
    t0.step(g1)
    t0.step(g2)
    assert calls == ["msclip_adamw_multi"] * 2
    del calls[:]
    t1 = train.TrainStep(_fresh(), lr=1e-3, bn="frozen", clip_grad_norm=1.0, optimizer="lamb", ema_decay=0.5)
    t1.step(g1)
    assert calls == ["msclip_grad_sumsq", "msclip_clip_coef", "msclip_lamb_partials", "msclip_lamb_ratios", "msclip_lamb_apply",
                     "msclip_ema_multi"] and not set(calls) & set(ext4)
    assert t1._skip_event is None and t1._skip_host is None              # nothing queued, nothing to wait for
    del calls[:]
    t2 = train.TrainStep(_fresh(), lr=1e-3, bn="frozen", nonfinite="skip", clip_grad_norm=1.0, optimizer="lamb", ema_decay=0.5)
    t2.step(g1)
    assert calls == ["msclip_grad_sumsq", "msclip_clip_coef_guarded", "msclip_lamb_partials", "msclip_lamb_ratios",
                     "msclip_lamb_apply_guarded", "msclip_ema_multi"]
    del calls[:]
    t3 = train.TrainStep(_fresh(), lr=1e-3, bn="frozen", nonfinite="skip")
    t3.step(g1)
    assert calls == ["msclip_grad_sumsq", "msclip_clip_coef_guarded", "msclip_adamw_multi_guarded"]
    # from_config passes the setting on
    cfg = named_config(B32, ["MODEL.SPEC.PRECISION", "bf16", "TRAIN.DETECT_ANOMALY", "True"])
    assert train.from_config(_fresh(), cfg, bn="frozen").nonfinite == "raise"
    assert train.from_config(_fresh(), named_config(B32, ["MODEL.SPEC.PRECISION", "bf16"]), bn="frozen").nonfinite is None
