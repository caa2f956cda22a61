"""Every cross-stream tensor hand-off of the eager training / forward step is ordered by an event, and every tensor that crosses a
stream is known to the caching allocator there: tests/stream_order.py's recorder around the real steps, its checker over the
record.  Batch 4, synthetic weights and inputs, plan=False (a replayed launch table never enters Python: the check covers the
eager loop the table is recorded from).  Each case is traced on its SECOND call, after a warm-up that allocates workspaces,
weight caches and lazy tables, and must come out with no violation and no unresolved access.

Also here: the write table against observation (an argument whose bytes a call changed must be declared written), and the checker's
teeth on the real record (one hand-off's wait, one record_stream deleted offline: both must be reported at that hand-off)."""
import pytest
import torch

import stream_order as so
from conftest import set_opt, synth_sd
from msclip_amd import gradgemm, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
B32, L14, B = "b32-yfcc-msclips", "l14-fp8-msclips", 4


def _fresh(name):
    m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", "bf16"]))
    m.load_state_dict(synth_sd(name), strict=True)
    return m.cuda().eval()


def _inputs(n=B):
    return synth.synth_images(n, seed=51).cuda(), synth.synth_tokens(n, seed=52).cuda()


def _traced(name, once, warm=True):
    """once() twice, the second time under the recorder -> the Trace (counts printed for profiles/stream_order_check.md)."""
    if warm:
        once()
    torch.cuda.synchronize()
    with so.Recorder() as rec:
        once()
    torch.cuda.synchronize()
    rep = so.check(rec.trace)
    print(f"{name}: {rec.trace.counts()}, cross-stream pairs checked {rep.pairs}, violations {len(rep.violations)}, "
          f"unresolved {len(rep.unresolved)}")
    return rec.trace, rep


def _train_step(monkeypatch, bn):
    m = _fresh(B32)
    ts = train.TrainStep(m, lr=1e-4, bn=bn)
    set_opt(monkeypatch, m, plan=False)
    img, tok = _inputs()

    def once():
        ts.forward(img, tok)
        ts.step(ts.backward())
    return ts, once


_TRAIN = {}


def _train_trace(monkeypatch):
    """The frozen-statistics step's record: made once, shared by the traced case and the two offline deletions."""
    if "frozen" not in _TRAIN:
        ts, once = _train_step(monkeypatch, "frozen")
        assert gradgemm.lane_enabled()
        _TRAIN["frozen"] = _traced("train b32 bn=frozen", once)
    return _TRAIN["frozen"]


def _assert_clean(rep):
    assert rep.clean(), rep.text()
    assert rep.pairs > 0                                      # (something did cross a stream)


# ---------------------------------------------------------------------------------------------------------------------
# the traced cases
# ---------------------------------------------------------------------------------------------------------------------
def test_training_step_frozen_statistics(gpu_device, monkeypatch):
    trace, rep = _train_trace(monkeypatch)
    lane = gradgemm.lane(gpu_device).cuda_stream
    on_lane = {e[1] for e in trace.events if e[0] == "access" and e[2] == lane}
    assert {"im2col", "colsum", "bn_fold_bwd"} <= on_lane, on_lane          # both conv-side job kinds run there (the defaults)
    assert any(e[1] == "AdamwPlan.run" for e in trace.events if e[0] == "access")
    _assert_clean(rep)


def test_training_step_batch_statistics(gpu_device, monkeypatch):
    _, once = _train_step(monkeypatch, "batch")
    _assert_clean(_traced("train b32 bn=batch", once)[1])


def test_accumulate_over_two_chunks(gpu_device, monkeypatch):
    m = _fresh(B32)
    ts = train.TrainStep(m, lr=1e-4, bn="frozen")
    set_opt(monkeypatch, m, plan=False)
    img, tok = _inputs(2 * B)
    chunks = [(img[:B], tok[:B]), (img[B:], tok[B:])]
    _assert_clean(_traced("accumulate b32 2 x 4", lambda: ts.accumulate(chunks))[1])


def test_engine_run_with_both_side_streams(gpu_device, monkeypatch):
    eng = set_opt(monkeypatch, _fresh(B32), plan=False, conv_side_stream=True, text0_stream=True)
    img, tok = _inputs()
    trace, rep = _traced("Engine.run b32", lambda: eng.run(img, tok))
    assert rep.pairs > 0 and trace.counts()["streams"] >= 3
    _assert_clean(rep)


def test_engine_run_patch_stem_model(gpu_device, monkeypatch):
    eng = set_opt(monkeypatch, _fresh(L14), plan=False)
    img, tok = _inputs()
    rep = _traced("Engine.run l14 bf16", lambda: eng.run(img, tok))[1]
    assert rep.clean(), rep.text()


def test_captions_staged_on_a_prefetch_stream(gpu_device, monkeypatch):
    """The hand-off of tests/test_gpu_pack.py::test_captions_staged_on_a_prefetch_stream: a batch staged on another stream than
    the one that consumes it, dropped right after the call, the next allocation made on the staging stream at once."""
    eng = set_opt(monkeypatch, _fresh(B32), plan=False)
    img, tok = _inputs()
    prefetch = torch.cuda.Stream()

    def once():
        prefetch.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(prefetch):
            cap = eng.stage_captions(tok.clone())
        torch.cuda.current_stream().wait_stream(prefetch)
        w = eng.run(img, cap)
        del cap
        with torch.cuda.stream(prefetch):
            junk = [torch.full((B + 2,), -1, dtype=torch.int32, device="cuda") for _ in range(8)]
        del junk
        return w
    trace, rep = _traced("staged captions b32", once)
    assert any(e[0] == "record_stream" for e in trace.events)
    _assert_clean(rep)


# ---------------------------------------------------------------------------------------------------------------------
# the write table against observation
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def _observed_writes(run):
    """run() under a recorder whose hook clones the tensor arguments of every top-level binding call, synchronizes, lets the call
    run, synchronizes and compares -> [(function, argument)] whose bytes changed without the table declaring them written (an
    argument that shares bytes with a declared one -- an in-place residual -- is that one)."""
    undeclared, calls = [], [0]

    def observe(name, tensors):
        live = [(p, t) for p, t in tensors if t.is_cuda and t.numel()]
        declared = [so.interval(t) for p, t in live if so.is_write(name, p)]
        torch.cuda.synchronize()
        before = [(p, t, _bits(t).clone()) for p, t in live if not so.is_write(name, p)]
        calls[0] += 1

        def after():
            torch.cuda.synchronize()
            for p, t, was in before:
                lo, hi = so.interval(t)
                if not torch.equal(was, _bits(t)) and not any(a < hi and lo < b for a, b in declared):
                    undeclared.append((name, p))
        return after
    with so.Recorder(observe=observe):
        run()
    torch.cuda.synchronize()
    return undeclared, calls[0]


def test_write_table_against_observation(gpu_device, monkeypatch):
    """Every argument whose bytes a top-level binding call changed is declared in stream_order.WRITES: a missing entry would turn
    a write into a read and hide a race.  First call of a fresh TrainStep / engine, so that output buffers are not in their
    final state yet (and the test fixture has filled free memory with NaN).  What this cannot see: a kernel that rewrites
    identical bytes, and a write into an argument that overlaps a declared one."""
    _, once = _train_step(monkeypatch, "frozen")
    undeclared, n_train = _observed_writes(once)
    assert n_train > 300 and not undeclared, sorted(set(undeclared))
    eng = set_opt(monkeypatch, _fresh(B32), plan=False)
    img, tok = _inputs()
    undeclared, n_run = _observed_writes(lambda: eng.run(img, tok))
    assert n_run > 100 and not undeclared, sorted(set(undeclared))
    print(f"write table observed over {n_train} + {n_run} top-level calls")


# ---------------------------------------------------------------------------------------------------------------------
# teeth, on the real record (nothing runs on the GPU here beyond making the record)
# ---------------------------------------------------------------------------------------------------------------------
def _lane_handoff(trace, lane):
    """The first hip.forked hand-off to the lane (an event recorded on another stream, the lane's wait for it right behind) whose
    job starts by reading bytes that another stream wrote earlier in the record -- the weight transposes at the top of the
    backward read only what the previous step left.  -> (index of the wait_event, the lane's first launch behind it as the
    checker names it).  Chosen from the record's own facts, not from what the checker says."""
    ev = trace.events
    written = []                                             # byte intervals written so far on other streams than the lane
    i = 0
    while i < len(ev):
        e = ev[i]
        if e[0] == "access" and e[2] != lane:
            written += [(lo, hi) for _, lo, hi in e[4]]
        if (e[0] == "wait_event" and e[1] == lane and ev[i - 1][0] == "record" and ev[i - 1][1] == e[2] and ev[i - 1][2] != lane):
            first = next(k for k in range(i, len(ev)) if ev[k][0] == "access" and ev[k][2] == lane and "." not in ev[k][1])
            if any(a < hi and lo < b for _, lo, hi in ev[first][3] for a, b in written):
                n = sum(1 for x in ev[:first] if x[0] == "access" and x[1] == ev[first][1])
                return i, f"{ev[first][1]}#{n}("
        i += 1
    raise AssertionError("no hand-off to the lane in the record")


def test_a_deleted_wait_is_reported_at_its_hand_off(gpu_device, monkeypatch):
    trace, rep = _train_trace(monkeypatch)
    assert rep.clean(), rep.text()
    lane = gradgemm.lane(gpu_device).cuda_stream
    at, named = _lane_handoff(trace, lane)
    broken = so.check(trace.without(at))
    hits = [v for v in broken.violations if v.startswith("A ") and named in v and f"stream {lane:#x}" in v]
    assert hits, (named, broken.text()[:2000])
    print(f"deleted wait_event #{at}: {len(broken.violations)} violations, first: {hits[0]}")


def test_a_deleted_record_stream_is_reported_at_its_hand_off(gpu_device, monkeypatch):
    trace, rep = _train_trace(monkeypatch)
    assert rep.clean(), rep.text()
    lane = gradgemm.lane(gpu_device).cuda_stream
    ev = trace.events
    made = {}                                                # storage -> the stream it was last allocated under, in the record
    told = {}                                                # storage -> indices of its record_stream(lane)
    for i, e in enumerate(ev):
        if e[0] == "alloc":
            made[(e[2], e[3])] = e[1]
            told.pop((e[2], e[3]), None)
        elif e[0] == "record_stream" and e[3] == lane:
            told.setdefault((e[1], e[2]), []).append(i)
    # a temporary of another stream that hip.forked told the allocator about exactly once
    (lo, hi), (rs,) = next((k, v) for k, v in told.items() if len(v) == 1 and made.get(k, lane) != lane)
    broken = so.check(trace.without(rs))
    assert broken.violations and all(v.startswith("B lifetime") for v in broken.violations), broken.text()[:2000]
    assert all(f"[{lo:#x}, {hi:#x})" in v and f"record_stream({lane:#x})" in v for v in broken.violations), broken.text()[:2000]
    print(f"deleted record_stream #{rs}: {broken.violations[0]}")
