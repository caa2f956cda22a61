"""The weight EMA (TRAIN.EMA_DECAY) on a real MI355X: msclip_ema_multi on a ragged list of misaligned views and across the
chunk-slot limit of a launch, TrainStep(ema_decay=...) over three steps of the B/32 model beside a twin without EMA,
ema_weights(), accumulate() and the checkpoint's 'ema_shadow_states'.

Reference: `decay * shadow + (1. - decay) * param` on fp32 torch tensors on the same device -- three kernels, three roundings.
Every comparison is exact (bit patterns): the update is three IEEE operations in a defined order, there is no tolerance."""
import pytest
import torch

from conftest import synth_sd
from msclip_amd import hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
B32 = "b32-yfcc-msclips"
CHUNK = 32768
# below, at and above one float4, one 256-thread sweep, one 32 K chunk and two chunks
COUNTS = [1, 2, 3, 4, 5, 7, 255, 256, 257, 32767, 32768, 32769, 65541]
N_TENSORS = 40                                               # more than one launch's tensor table (36)
GUARD = 0x7FC0BEEF                                           # a quiet NaN with a payload, as int32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _carve(counts, shifts, gen):
    """-> (arena, views, mask): views[i] = counts[i] randn elements that start shifts[i] * 4 bytes past a 16-byte boundary of
    one arena whose every other word (at least one between two tensors, four in front) holds the GUARD pattern."""
    starts, o = [], 4
    for n, sh in zip(counts, shifts):
        o = (o + 3) // 4 * 4 + sh
        starts.append(o)
        o += n + 1
    arena = torch.empty(o + 4, dtype=torch.float32, device="cuda")
    assert arena.data_ptr() % 16 == 0
    arena.view(torch.int32).fill_(GUARD)
    mask = torch.zeros(arena.numel(), dtype=torch.bool, device="cuda")
    views = []
    for n, st, sh in zip(counts, starts, shifts):
        v = arena[st:st + n]
        v.copy_(torch.randn(n, device="cuda", generator=gen))
        mask[st:st + n] = True
        assert v.data_ptr() % 16 == 4 * sh
        views.append(v)
    return arena, views, mask


def _guards_intact(arena, mask):
    return bool((arena.view(torch.int32)[~mask] == GUARD).all())


def _reference(shadows, params, decay):
    return [decay * s + (1. - decay) * p for s, p in zip(shadows, params)]


# ---------------------------------------------------------------------------- 1. the kernel
def test_ragged_list_of_misaligned_views(gpu_device):
    gen = torch.Generator(device="cuda").manual_seed(11)
    counts = [COUNTS[i % len(COUNTS)] for i in range(N_TENSORS)]
    s_shift = [i % 4 for i in range(N_TENSORS)]
    co = [(i // 4) % 2 == 0 for i in range(N_TENSORS)]                 # shadow and parameter at the same offset within 16 bytes
    p_shift = [sh if c else (sh + 1 + i // 8 % 3) % 4 for i, (sh, c) in enumerate(zip(s_shift, co))]
    assert sum(co) == N_TENSORS // 2 and all((a == b) == c for a, b, c in zip(s_shift, p_shift, co))
    for cls in (True, False):                                          # every alignment and a multi-chunk tensor in both classes
        assert {sh for sh, c in zip(s_shift, co) if c == cls} == {0, 1, 2, 3}
        assert any(n == 65541 for n, c in zip(counts, co) if c == cls)
    s_arena, shadows, s_mask = _carve(counts, s_shift, gen)
    p_arena, params, p_mask = _carve(counts, p_shift, gen)
    p_before = p_arena.clone()
    want = _reference(shadows, params, 0.999)
    # the reference is sensitive to the rounding order: rounding once instead of three times gives other bits
    big = counts.index(65541)
    once = (0.999 * shadows[big].double() + (1. - 0.999) * params[big].double()).float()
    assert not _same_bits(want[big], once)
    hip.ema_update(shadows, params, 0.999)
    torch.cuda.synchronize()
    for i, (s, w) in enumerate(zip(shadows, want)):
        assert _same_bits(s, w), (i, counts[i], s_shift[i], p_shift[i], (s - w).abs().max().item())
    assert _same_bits(p_arena, p_before)                               # parameters and their guard words
    assert _guards_intact(s_arena, s_mask) and _guards_intact(p_arena, p_mask)
    # decay 0: the shadow becomes the parameter
    plan = hip.EmaPlan(shadows, params)
    plan.run(0.0)
    torch.cuda.synchronize()
    for i, (s, p) in enumerate(zip(shadows, params)):
        assert _same_bits(s, p), (i, counts[i])
    assert _same_bits(p_arena, p_before) and _guards_intact(s_arena, s_mask)
    # empty tensors take no part; unequal counts are refused
    hip.ema_update([shadows[0][:0], shadows[6]], [params[0][:0], params[6]], 0.5)
    assert _same_bits(shadows[6], params[6]) and _guards_intact(s_arena, s_mask)
    with pytest.raises(AssertionError):
        hip.EmaPlan([shadows[5]], [params[6]])
    with pytest.raises(ValueError):
        plan.run(1.0)


def test_tensor_that_continues_in_the_next_launch(gpu_device):
    """A launch holds 768 chunks: behind a small tensor, one of 768 + 2 chunks fills the first launch's remaining 767 slots
    and restarts in the second at local chunk 0 with shifted bases."""
    gen = torch.Generator(device="cuda").manual_seed(12)
    counts = [5, 768 * CHUNK + CHUNK + 5]
    s_arena, shadows, s_mask = _carve(counts, [2, 1], gen)
    p_arena, params, p_mask = _carve(counts, [3, 1], gen)
    p_before = p_arena.clone()
    want = _reference(shadows, params, 0.999)
    hip.ema_update(shadows, params, 0.999)
    torch.cuda.synchronize()
    for s, w in zip(shadows, want):
        assert _same_bits(s, w), (s.numel(), (s - w).abs().max().item())
    assert _guards_intact(s_arena, s_mask) and _guards_intact(p_arena, p_mask)
    assert _same_bits(p_arena, p_before)


# ---------------------------------------------------------------------------- 2. the training step
def _fresh(name=B32, sd=None):
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(name) if sd is None else sd, strict=True)
    return m.cuda().eval()


def _batch(n, seed):
    return synth.synth_images(n, seed=seed).cuda(), synth.synth_tokens(n, seed=seed + 100).cuda()


def _params(m):
    return {k: p.detach().clone() for k, p in m.named_parameters()}


def _differ(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not _same_bits(a[k], b[k])]


@pytest.fixture(scope="module")
def trained(gpu_device):
    """Twin B/32 models from the same synthetic state, three steps at batch 8 with frozen statistics: (model with
    ema_decay = 0.5, its TrainStep, twin without EMA, its TrainStep).  Both twins step on the SAME gradient tensors, those of
    the EMA twin's backward (the embedding gradient's atomics make two backward passes differ in the last bits), so every
    bitwise comparison between them holds.  What is checked after every step is checked here; the tests below leave the
    four objects as they find them."""
    ma, mb = _fresh(), _fresh()
    ta = train.TrainStep(ma, lr=1e-4, bn="frozen", ema_decay=0.5)
    tb = train.TrainStep(mb, lr=1e-4, bn="frozen")
    assert tb.ema_shadow is None and tb.ema_decay is None and ta.ema_decay == 0.5 and ta.ema_updates == 0
    names = [k for k, _ in ma.named_parameters()]
    assert list(ta.ema_shadow) == names and len(names) == 325 and "logit_scale" in names
    assert not any(k.startswith("transformer.resblocks.5.mlp") for k in names)          # the text-tower aliases: no entry of their own
    ref = _params(ma)
    assert not _differ(ref, ta.ema_shadow)                             # every shadow starts as a copy of its parameter
    assert all(v.data_ptr() % 256 == 0 and v.dtype == torch.float32 for v in ta.ema_shadow.values())
    for step in range(1, 4):
        ta.forward(*_batch(8, 60 + step))
        grads = ta.backward()
        ta.step(grads)
        tb.step(grads)
        now = _params(ma)
        ref = {k: 0.5 * ref[k] + (1. - 0.5) * now[k] for k in names}   # the recurrence on this step's parameter values
        assert not _differ(ref, ta.ema_shadow), (step, _differ(ref, ta.ema_shadow)[:8])
        assert ta.ema_updates == step == ta.steps and tb.ema_updates == 0
        # the EMA does not perturb training: parameters and both AdamW moments of the twins
        assert not _differ(now, _params(mb)), (step, _differ(now, _params(mb))[:8])
        for i in (0, 1):
            sa, sb = ({k: st[i] for k, st in ts.state.items()} for ts in (ta, tb))
            assert not _differ(sa, sb), (step, i, _differ(sa, sb)[:8])
    assert _differ(ref, now)                                           # ... and the shadows are not the parameters
    return ma, ta, mb, tb


def test_shadows_follow_the_recurrence_and_training_is_unperturbed(trained):
    ma, ta, mb, tb = trained                                           # (the fixture asserts after every step)
    assert ta.ema_updates == 3 and ta.steps == 3 and tb.steps == 3
    on = train.from_config(mb, named_config(B32, ["TRAIN.EMA_DECAY", "0.25"]), bn="frozen")
    assert on.ema_decay == 0.25 and not _differ(_params(mb), on.ema_shadow)
    off = train.from_config(mb, named_config(B32, ["TRAIN.EMA_DECAY", "0.0"]), bn="frozen")
    assert off.ema_decay is None and off.ema_shadow is None
    assert train.from_config(mb, named_config(B32), bn="frozen").ema_shadow is None


def test_ema_weights_context(trained):
    ma, ta, _, tb = trained
    img, tok = _batch(8, 70)
    live, shadow = _params(ma), {k: v.clone() for k, v in ta.ema_shadow.items()}
    logits_live = ma(img, tok).clone()
    # a fresh model loaded with the shadow values (every state_dict key of a Parameter, aliases included; buffers as they are)
    name_of = {id(p): k for k, p in ma.named_parameters()}
    sd = {k: (shadow[name_of[id(t)]] if id(t) in name_of else t.detach()).cpu().clone()
          for k, t in ma.state_dict(keep_vars=True).items()}
    mf = _fresh(sd=sd)
    logits_shadow = mf(img, tok).clone()
    assert not _same_bits(logits_shadow, logits_live)
    with ta.ema_weights() as inside:
        assert inside is ta
        assert not _differ(_params(ma), shadow)                        # the model holds the shadow values ...
        assert not _differ(dict(ta.ema_shadow), live)                  # ... and the arena the live ones
        assert _same_bits(ma(img, tok), logits_shadow)
        for call in (lambda: ta.step({}), lambda: ta.forward(img, tok), lambda: ta.accumulate([(img, tok)]), ta.ema_assign):
            with pytest.raises(RuntimeError, match="ema_assign"):
                call()
    assert not _differ(_params(ma), live)
    assert not _differ(dict(ta.ema_shadow), shadow)
    assert _same_bits(ma(img, tok), logits_live)
    with pytest.raises(RuntimeError):
        ta.ema_resume()                                                # nothing assigned
    with pytest.raises(RuntimeError):
        tb.ema_assign()                                                # no EMA
    assert ta.ema_updates == 3 and ta.steps == 3


def test_accumulate_updates_the_ema_once_per_step(gpu_device):
    m = _fresh()
    ts = train.TrainStep(m, lr=2e-5, bn="frozen", ema_decay=0.5)
    img, tok = _batch(8, 80)
    before = _params(m)
    _, grads = ts.accumulate([(img[:4], tok[:4]), (img[4:], tok[4:])])
    assert ts.ema_updates == 0 and not _differ(before, ts.ema_shadow)
    ts.step(grads)
    assert ts.ema_updates == 1
    now = _params(m)
    want = {k: 0.5 * before[k] + (1. - 0.5) * now[k] for k in before}
    assert not _differ(want, ts.ema_shadow) and _differ(before, now)
    # training goes on behind ema_weights(): the optimizer's table is rebuilt over the re-packed engine, the shadows follow
    with ts.ema_weights():
        assert not _differ(_params(m), want)
    ts.forward(img, tok)
    ts.step(ts.backward())
    after = _params(m)
    assert ts.ema_updates == 2 and _differ(now, after)
    assert not _differ({k: 0.5 * want[k] + (1. - 0.5) * after[k] for k in want}, ts.ema_shadow)


def test_checkpoint_carries_the_shadows(trained, tmp_path):
    ma, ta, _, _ = trained
    on, off = tmp_path / "ema_on.pth", tmp_path / "ema_off.pth"
    train.save_checkpoint(ma, ta, on, step=2, model_name=B32)
    mc = _fresh()
    tc = train.TrainStep(mc, lr=1e-4, bn="frozen", ema_decay=0.5)
    td = train.TrainStep(mc, lr=1e-4, bn="frozen")
    train.save_checkpoint(mc, td, off, step=0, model_name=B32)         # (no step taken: no moments, a small file)
    obj = torch.load(off, weights_only=False)
    assert set(obj) == {"step", "model", "state_dict", "perf", "optimizer"}
    with pytest.raises(KeyError, match="ema_shadow_states"):
        train.resume_checkpoint(mc, tc, off)                           # the reference asserts the key (lib/utils/utils.py:130)
    del obj
    assert train.resume_checkpoint(mc, tc, on) == 3 and tc.steps == 3
    assert list(tc.ema_shadow) == list(ta.ema_shadow) and not _differ(dict(tc.ema_shadow), dict(ta.ema_shadow))
    assert not _differ(_params(mc), _params(ma)) and _differ(_params(mc), dict(tc.ema_shadow))
    obj = torch.load(on, weights_only=False)
    assert set(obj) == {"step", "model", "state_dict", "perf", "optimizer", "ema_shadow_states"}
    assert list(obj["ema_shadow_states"]) == list(ta.ema_shadow)
    assert all(not v.is_cuda and v.dtype == torch.float32 for v in obj["ema_shadow_states"].values())
    del obj
    assert train.resume_checkpoint(mc, td, on) == 3 and td.ema_shadow is None      # EMA off: the key is ignored
