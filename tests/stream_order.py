"""Happens-before check of the cross-stream tensor hand-offs of the eager training / forward step.  An ordinary module, in the
manner of tests/gradcheck.py: no fixtures, no pytest hooks, importable without a GPU.  Shared by tests/test_stream_order_cpu.py
(the checker against hand-written traces) and tests/test_gpu_stream_order.py (the real steps, recorded on the device).

Three parts:

  Recorder   a context manager that records, in issue order, (a) every call of a public function of msclip_amd.hip -- nested
             calls too -- and of the run() of its table classes (AdamwPlan, AccumulatePlan, ...), every tensor as the byte interval
             [data_ptr, data_ptr + extent) with the extent taken from shape, stride and itemsize, the fields of FoldIn / FoldOut /
             QkvAttnTables and tensors inside lists and tuples followed; (b) every ATen op through a TorchDispatchMode: its tensor
             arguments, which the schema marks written, which outputs are fresh allocations (a storage none of the inputs has),
             aten.record_stream; (c) Event.record / wait / synchronize, Stream.wait_event / wait_stream / record_event /
             synchronize and torch.cuda.synchronize.  Everything is restored on exit.
  WRITES     {hip function: the arguments (or descriptor fields, dotted; "*" = any list index; "return" = tensors the call
             hands back that are none of its arguments) it writes}.  Every other tensor argument is a read.  EXTENTS narrows an
             argument that is passed whole but touched in part, from the call's own arguments: the only form of waiver.  None:
             the function takes tensors but looks at their shapes only and launches nothing (what ATen ops it runs are
             recorded as such).
  check()    vector clocks per stream over the recorded events.  Check A (ordering): two accesses to overlapping bytes on
             different streams, at least one a write, need a happens-before path (RAW, WAR, WAW).  Check B (lifetime): a fresh
             allocation clears the shadow state of its bytes -- the caching allocator orders reuse within the allocating stream --
             and in exchange every storage allocated under stream S and accessed on T != S must have had record_stream(T) by
             the end of the trace, or be persistent (alive before the trace began and still alive at its end: weights,
             workspaces, optimizer state).  A storage that is older than the trace but dies inside it counts as allocated under
             the stream that was current when the trace began.

Edges: Event.record snapshots the recording stream's clock; wait_event joins the LAST snapshot taken before the wait (an event
never recorded gives no edge); wait_stream joins the other stream's clock; a host-side synchronize (torch.cuda.synchronize,
Stream / Event.synchronize, and the ops that block the host on the current stream: .item(), a blocking copy to the host) joins
what it waits for into every stream's later work.

Limits, by construction:
  * the launch-table replay (plan=True) never enters Python: the check covers the eager loop the table is recorded from, not the
    table's own stream edges;
  * host-side hazards are not modelled (pinned staging buffers, the decode worker): accesses to host memory are left out;
  * RCCL collectives are opaque calls on their stream that read `send` and write `recv`;
  * a kernel's access is the whole (or EXTENTS-narrowed) interval of its argument: two launches that interleave rows or column
    windows of one buffer need an extent function, which cites the line that fixes the ranges;
  * the implicit synchronisation of the legacy default stream with blocking streams is not an edge here (every stream of this
    project is non-blocking), so a step that relied on it would be reported.
"""
import bisect
import contextlib
import inspect

import torch

from msclip_amd import hip

# ---------------------------------------------------------------------------------------------------------------------
# the write table
# ---------------------------------------------------------------------------------------------------------------------
RETURN = "return"
WRITES = {
    "allgather_feats": ("recv",),
    "allreduce": ("t",),
    "gemm": ("out", "out2", "fold_out.xb", "fold_out.part", "colsum_part", "bn_stats_part"),
    "quantize_rows_f8": (RETURN,),
    "gemm_f8": ("out", "fold_out.xb", "fold_out.part"),
    "layernorm_f8": ("q", "row_scale"),
    "quant_f8_rows": ("q", "row_scale"),
    "gemm_splitk": ("out", RETURN),
    "gemm_splitk_tn": ("out", RETURN),
    "ktab_taps": None,
    "attention": ("out",),
    "attention_lastq": ("out",),
    "layernorm": ("out", "raw_out"),
    "layernorm_stats": ("out", "raw_out", "center", "rowstat"),
    "rowstat_finalize": ("center", "rowstat"),
    "layernorm_split": ("out",),
    "embed_tokens": ("x", "eot_row"),
    "text_lengths": ("length", "cu", "eot_row", "dims"),
    "embed_tokens_packed": ("x",),
    "attention_varlen": ("out",),
    "attention_lastq_varlen": ("out",),
    "head_major_qkv": (RETURN,),
    "qkv_attention": ("out",),
    "fill_cls": ("x",),
    "adapter_combine_ln": ("xout",),
    "adapter_combine_ln_stats": ("xout", "lno", "center", "rowstat"),
    "patchify": ("out",),
    "l2norm": ("out_f32", "out_bf16"),
    "gather_rows": ("out",),
    "stem_conv_dual": ("out_a", "out_b"),
    "stem_conv_dual_raw": ("out_a", "out_b"),
    "stem_conv_dual_bn": ("y_a", "y_b", "xhat_a", "xhat_b", RETURN),
    "stem_dual_conv3x3s2": ("out_b", "out2"),
    "conv1x1_conv3x3s2": ("out",),
    "convresblock48_s2": ("out",),
    "dwpool": ("out",),
    "lse_rows": ("lse",),
    "clip_loss_partial": ("out",),
    "clip_lse_fused": ("part_max", "part_sum", "diag"),
    "clip_loss_from_partials": ("out", "lse_out"),
    "transpose_bf16": (RETURN,),
    "cast_bf16": ("out", RETURN),
    "cast_bf16_colsum": ("out", RETURN),
    "colsum": ("out", RETURN),
    "quickgelu": ("y",),
    "quickgelu_bwd": ("dh",),
    "layernorm_bwd": ("dx", "dxb", "sum_part", RETURN),
    "attention_bwd": ("dqkv", "colsum_part"),
    "attention_bwd_varlen": ("dqkv", "colsum_part"),
    "embed_tokens_bwd_packed": ("demb", "dpos"),
    "l2norm_bwd": ("dx",),
    "clip_loss_bwd_g": ("G", "dscale_part"),
    "embed_tokens_bwd": ("demb", "dpos"),
    "adapter_sum": ("out",),
    "adapter_dx": ("dx",),
    "im2col": (RETURN,),
    "image_conv_wgrad_ok": None,
    "image_conv_wgrad": (RETURN,),
    "col2im": ("dx",),
    "relu_bwd": ("out", RETURN),
    "dwpool_bwd": ("dtop",),
    "dwpool_wgrad": (RETURN,),
    "dw3x3_wgrad": (RETURN,),
    "bn_stats": (RETURN,),
    "bn_stats_partials": (RETURN,),
    "bn_bwd_token_columns": ("dx", RETURN),
    "bn_finish": ("out",),
    "bn_apply": ("out",),
    "bn_bwd": ("dx", RETURN),
    "bn_bwd_fused_ok": None,
    "bn_bwd_fused": ("sides.*.4", RETURN),
    "bn_fold_bwd": (RETURN,),
    "adamw_multi": ("items.*.0", "items.*.2", "items.*.3", "items.*.6"),
    "grad_norm": (RETURN,),
    "adamw": ("p", "m", "v"),
    "grad_accumulate": ("accs",),
    "ema_update": ("shadows",),
    "split_bf16": ("out", RETURN),
    "probe_ce_rows": ("lse", "G_hi", "G_lo", "loss_part", "colsum_part", "pred", "rank", "bad_part"),
    "probe_loss_fold": ("out",),
}
# public functions of msclip_amd.hip that take no tensor (streams, build, probes' switches).  A call of one of them that is
# handed a tensor all the same is reported as unresolved.
NO_TENSORS = frozenset((
    "build", "lib", "env_flag", "require_gpu", "zero_page", "off_default_stream", "use_compute_stream", "priority_stream",
    "background_stream", "compute_stream", "cu_masked_stream", "gemm_variant", "describe_gemm", "gemm_bn_two_pass_ok",
    "python_probes_active", "set_gemm_probe", "set_wg_cap", "set_gemm_f8_probe"))


def _row_range(rows_of):
    """Extent function: rows [r0, r1) = rows_of(tensor, bound arguments) of a 2-D argument that is passed whole."""
    def extent(t, args):
        r = rows_of(t, args)
        if r is None or t.dim() != 2 or not 0 <= r[0] < r[1] <= t.shape[0]:
            return None
        return t[r[0]:r[1]]
    return extent


def _gemm_out_rows(out, a):
    """include/msclip_hip.h, msclip_gemm_desc: output row of GEMM row m = m + (m / rpg) * radd + roff, m < M (rpg = INT_MAX,
    radd = roff = 0: the identity).  Row arithmetic is in units of ldo: only where that is the tensor's own row stride."""
    if a.get("bn_stats_part") is not None or (a.get("ldo") is not None and a["ldo"] != out.stride(0)):
        return None
    M = a["M"] if a.get("M") is not None else (a["x"].shape[0] if a.get("conv") is None else None)
    if M is None or M < 1:
        return None
    return a["roff"], (M - 1) + ((M - 1) // a["rpg"]) * a["radd"] + a["roff"] + 1


# {function: {argument path: extent function(tensor, bound arguments) -> the part of the tensor the launch touches, or None}}.
# One entry per report that turned out to be two launches on disjoint rows of one buffer; each cites what fixes the rows.
EXTENTS = {
    # Engine._run_body: the text front + text block 0 on the text-0 stream beside the image front on the main stream, both
    # handed the whole token matrix w["X"].  Engine._tokenise (engine.py, `hip.gemm(x, ..., w["X"], M=Bi * g2, ..., rpg=g2,
    # radd=1, roff=1)`) scatters to the image rows b * Lv + 1 + p < Mv; Engine._text_front passes row_base = w["Mv"]
    "gemm": {"out": _row_range(_gemm_out_rows)},
    # the same hand-off, the next launch of Engine._tokenise (`hip.fill_cls(self.cls, self.vpos, w["X"], Bi, self.Lv)`);
    # include/msclip_hip.h, msclip_fill_cls: writes x[b * L], b < B
    "fill_cls": {"x": _row_range(lambda x, a: (0, (a["B"] - 1) * a["L"] + 1))},
    # include/msclip_hip.h, msclip_embed_tokens_packed: writes x[row_base + cu[b] + l] and zeroes up to row_base + rows_padded
    "embed_tokens_packed": {"x": _row_range(lambda x, a: (a["row_base"], a["row_base"] + a["rows_padded"]))},
    # include/msclip_hip.h, msclip_embed_tokens: writes x[row_base + b * L + l]
    "embed_tokens": {"x": _row_range(lambda x, a: (a["row_base"], a["row_base"] + a["tokens"].shape[0] * a["tokens"].shape[1]))},
}


def public_functions(module=hip):
    """{name: function} of the module's public functions: what the recorder wraps and what test_stream_order_cpu.py wants classified."""
    return {n: f for n, f in vars(module).items()
            if inspect.isfunction(f) and getattr(f, "__module__", None) == module.__name__ and not n.startswith("_")}


def unclassified(module=hip):
    """Public functions that are in neither WRITES nor NO_TENSORS, and entries of WRITES naming an argument the function does
    not have: both lists must be empty."""
    missing, bad = [], []
    for name, fn in public_functions(module).items():
        if name not in WRITES and name not in NO_TENSORS:
            missing.append(name)
        elif name in WRITES:
            params = inspect.signature(fn).parameters
            for path in WRITES[name] or ():
                head = path.split(".")[0]
                if head != RETURN and head not in params:
                    bad.append(f"{name}: {path}")
            for path in EXTENTS.get(name, {}):
                if path.split(".")[0] not in params:
                    bad.append(f"{name}: extent of {path}")
    return missing, bad


def _matches(path, spec):
    a, b = path.split("."), spec.split(".")
    return len(a) >= len(b) and all(y == "*" or x == y for x, y in zip(a, b))


def is_write(fn, path):
    return any(_matches(path, spec) for spec in WRITES.get(fn) or ())


# ---------------------------------------------------------------------------------------------------------------------
# the trace: plain tuples, so that a test can write one by hand
# ---------------------------------------------------------------------------------------------------------------------
def access(fn, stream, reads=(), writes=()):
    """A launch or ATen op on `stream`; reads / writes: {argument name: (lo, hi)} or [(name, lo, hi)] byte intervals."""
    def norm(x):
        return [(k, v[0], v[1]) for k, v in x.items()] if isinstance(x, dict) else list(x)
    return ("access", fn, stream, norm(reads), norm(writes), [])


def alloc(stream, lo, hi):
    return ("alloc", stream, lo, hi)


def record_stream(lo, hi, stream):
    return ("record_stream", lo, hi, stream)


def record(event, stream):
    return ("record", event, stream)


def wait_event(stream, event):
    return ("wait_event", stream, event)


def wait_stream(stream, other):
    return ("wait_stream", stream, other)


def synchronize(what=None):
    """Host-side: None = the device, ("stream", s) or ("event", e)."""
    return ("sync", what)


class Trace:
    """events: the tuples above, in issue order.  alive_start / alive_end: byte intervals of the device allocations that were live
    when the trace began / when it ended (persistent = inside both and never freshly allocated in between).  main: the stream
    that was current when the trace began."""

    def __init__(self, events=(), alive_start=(), alive_end=None, main=0):
        self.events, self.alive_start, self.main = list(events), list(alive_start), main
        self.alive_end = list(alive_start) if alive_end is None else list(alive_end)

    def without(self, index):
        return Trace(self.events[:index] + self.events[index + 1:], self.alive_start, self.alive_end, self.main)

    def counts(self):
        acc = [e for e in self.events if e[0] == "access"]
        streams = {e[2] for e in acc}
        launches = sum(1 for e in acc if "." not in e[1] or e[1].endswith(".run"))       # (an ATen op's name has its namespace)
        return dict(launches=launches, aten=len(acc) - launches, streams=len(streams),
                    events=len({e[1] for e in self.events if e[0] == "record"}))


# ---------------------------------------------------------------------------------------------------------------------
# interval map
# ---------------------------------------------------------------------------------------------------------------------
class _Segments:
    """Disjoint byte ranges [lo, hi) -> value, sorted.  span(lo, hi) cuts the ranges at lo and hi, fills the gaps with new()
    and returns the indices that cover exactly [lo, hi)."""

    def __init__(self, new, copy):
        self.lo, self.hi, self.val, self.new, self.copy = [], [], [], new, copy

    def _cut(self, at):
        i = bisect.bisect_right(self.lo, at) - 1
        if i >= 0 and self.lo[i] < at < self.hi[i]:
            self.lo.insert(i + 1, at)
            self.hi.insert(i + 1, self.hi[i])
            self.val.insert(i + 1, self.copy(self.val[i]))
            self.hi[i] = at

    def span(self, lo, hi):
        self._cut(lo)
        self._cut(hi)
        i = bisect.bisect_left(self.lo, lo)
        if i > 0 and self.hi[i - 1] > lo:
            i -= 1
        at, j = lo, i
        while at < hi:
            if j < len(self.lo) and self.lo[j] <= at:
                at = self.hi[j]
            else:
                end = min(hi, self.lo[j]) if j < len(self.lo) else hi
                self.lo.insert(j, at)
                self.hi.insert(j, end)
                self.val.insert(j, self.new())
                at = end
            j += 1
        return range(i, j)

    def assign(self, lo, hi, value):
        r = self.span(lo, hi)
        del self.lo[r.start:r.stop], self.hi[r.start:r.stop], self.val[r.start:r.stop]
        self.lo.insert(r.start, lo)
        self.hi.insert(r.start, hi)
        self.val.insert(r.start, value)

    def overlapping(self, lo, hi):
        i = bisect.bisect_right(self.lo, lo) - 1
        if i < 0 or self.hi[i] <= lo:
            i += 1
        out = []
        while i < len(self.lo) and self.lo[i] < hi:
            out.append(i)
            i += 1
        return out


class _Cover:
    """Is [lo, hi) inside one of these disjoint intervals?"""

    def __init__(self, intervals):
        iv = sorted(intervals)
        self.lo, self.hi = [a for a, _ in iv], [b for _, b in iv]

    def inside(self, lo, hi):
        i = bisect.bisect_right(self.lo, lo) - 1
        return i >= 0 and hi <= self.hi[i]


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.violations, self.unresolved, self.pairs = [], [], 0

    def clean(self):
        return not self.violations and not self.unresolved

    def text(self):
        return "\n".join(self.violations + ["unresolved: " + u for u in self.unresolved]) or "clean"


def check(trace):
    """-> Report.  violations: one line per (kind, pair of calls); unresolved: accesses the recorder could not classify."""
    rep = Report()
    clocks, base, snaps = {}, {}, {}

    def clock(s):
        if s not in clocks:
            clocks[s] = dict(base)
        return clocks[s]

    def join(into, other):
        for k, v in other.items():
            if into.get(k, 0) < v:
                into[k] = v

    def host_waits_for(vc):
        join(base, vc)
        for c in clocks.values():
            join(c, vc)

    shadow = _Segments(lambda: [None, {}], lambda v: [v[0], dict(v[1])])       # [last write, {stream: last read}]
    owners = _Segments(lambda: None, lambda v: v)                              # live allocations made inside the trace
    allocs, old, recorded_old, seen = [], [], [], set()
    at_start, at_end = _Cover(trace.alive_start), _Cover(trace.alive_end)
    ordinal = {}

    def name(a):
        return f"{a[0]}#{a[1]}({a[2]}, stream {a[3]:#x})"

    def flag(kind, first, second, lo, hi):
        key = (kind, first[0], first[1], first[2], second[0], second[1], second[2])
        if key not in seen:
            seen.add(key)
            rep.violations.append(f"A {kind}: {name(second)} is not ordered behind {name(first)}: bytes [{lo:#x}, {hi:#x})")

    def ordered(first, vc):
        return vc.get(first[3], 0) >= first[4]

    for ev in trace.events:
        kind = ev[0]
        if kind == "access":
            _, fn, s, reads, writes, unresolved = ev
            n = ordinal[fn] = ordinal.get(fn, -1) + 1
            for u in unresolved:
                rep.unresolved.append(f"{fn}#{n} on stream {s:#x}: {u}")
            vc = clock(s)
            vc[s] = tick = vc.get(s, 0) + 1
            for is_w, group in ((False, reads), (True, writes)):
                for arg, lo, hi in group:
                    if hi <= lo:
                        continue
                    me = (fn, n, arg, s, tick)
                    for i in shadow.span(lo, hi):
                        st = shadow.val[i]
                        w = st[0]
                        if w is not None and w[3] != s:
                            rep.pairs += 1
                            if not ordered(w, vc):
                                flag("WAW" if is_w else "RAW", w, me, shadow.lo[i], shadow.hi[i])
                        if is_w:
                            for r in st[1].values():
                                if r[3] != s:
                                    rep.pairs += 1
                                    if not ordered(r, vc):
                                        flag("WAR", r, me, shadow.lo[i], shadow.hi[i])
                            shadow.val[i] = [me, {}]
                        else:
                            st[1][s] = me
                    # lifetime: whose memory is it, and does its allocator know about this stream
                    own = [owners.val[i] for i in owners.overlapping(lo, hi) if owners.val[i] is not None]
                    for a in own:
                        if a["stream"] != s:
                            a["needs"].setdefault(s, me)
                    if not own and s != trace.main and not (at_start.inside(lo, hi) and at_end.inside(lo, hi)):
                        old.append((lo, hi, s, me))
        elif kind == "alloc":
            _, s, lo, hi = ev
            if hi > lo:
                a = dict(stream=s, lo=lo, hi=hi, needs={}, recorded=set())
                allocs.append(a)
                owners.assign(lo, hi, a)
                shadow.assign(lo, hi, [None, {}])
        elif kind == "record_stream":
            _, lo, hi, s = ev
            own = [owners.val[i] for i in owners.overlapping(lo, hi) if owners.val[i] is not None]
            for a in own:
                a["recorded"].add(s)
            if not own:
                recorded_old.append((lo, hi, s))
        elif kind == "record":
            snaps[ev[1]] = dict(clock(ev[2]))
        elif kind == "wait_event":
            if ev[2] in snaps:                                   # (never recorded: no edge)
                join(clock(ev[1]), snaps[ev[2]])
        elif kind == "wait_stream":
            join(clock(ev[1]), clock(ev[2]))
        elif kind == "sync":
            what = ev[1]
            if what is None:
                for c in list(clocks.values()):
                    host_waits_for(dict(c))
            elif what[0] == "stream":
                host_waits_for(dict(clock(what[1])))
            elif what[1] in snaps:
                host_waits_for(dict(snaps[what[1]]))
        else:
            raise ValueError(f"unknown trace event {ev!r}")
    for a in allocs:
        for s, me in a["needs"].items():
            if s not in a["recorded"]:
                rep.violations.append(f"B lifetime: {name(me)} reads or writes bytes [{a['lo']:#x}, {a['hi']:#x}) allocated under stream "
                                      f"{a['stream']:#x}, with no record_stream({s:#x}) and not persistent")
    told = set()
    for lo, hi, s, me in old:
        if not any(a < hi and lo < b and t == s for a, b, t in recorded_old) and (me[0], me[1], me[2]) not in told:
            told.add((me[0], me[1], me[2]))
            rep.violations.append(f"B lifetime: {name(me)} reads or writes bytes [{lo:#x}, {hi:#x}) that are older than the trace, die "
                                  f"inside it (allocated under stream {trace.main:#x}), with no record_stream({s:#x})")
    return rep


# ---------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------
def interval(t):
    """Byte interval [lo, hi) a strided tensor spans, from data_ptr(), shape, stride and itemsize; None for an empty one."""
    if t.numel() == 0:
        return None
    last = sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    lo = t.data_ptr()
    return lo, lo + (last + 1) * t.element_size()


def _storage(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def _raw_stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _stream_handle(s):
    """aten.record_stream's stream argument (a torch.Stream) -> the raw handle the other events carry."""
    return torch.cuda.Stream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type).cuda_stream


def _live_blocks():
    """Byte intervals of the caching allocator's live blocks."""
    out = []
    for seg in torch.cuda.memory_snapshot():
        at = seg["address"]
        for b in seg["blocks"]:
            if b["state"] == "active_allocated":
                out.append((at, at + b["size"]))
            at += b["size"]
    return out


_SCALARS = (bool, int, float, str, bytes, complex, torch.device, torch.dtype, torch.Size, torch.cuda.Stream, torch.cuda.Event)
_TABLES = ("AdamwPlan", "LambPlan", "AccumulatePlan", "EmaPlan", "PackPlan", "TransposePlan", "FoldPlan")


def walk(v, path, out, unresolved):
    """Every tensor inside an argument -> out [(dotted path, tensor)]; what cannot be followed -> unresolved."""
    if isinstance(v, torch.Tensor):
        out.append((path, v))
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            walk(x, f"{path}.{i}", out, unresolved)
    elif isinstance(v, dict):
        for k, x in v.items():
            walk(x, f"{path}.{k}", out, unresolved)
    elif v is None or isinstance(v, _SCALARS) or callable(v):
        pass
    elif type(v).__module__ == hip.__name__ and hasattr(v, "__dict__"):          # FoldIn / FoldOut / QkvAttnTables: their fields
        for k, x in vars(v).items():
            walk(x, f"{path}.{k}", out, unresolved)
    else:
        unresolved.append(f"argument {path} is a {type(v).__name__}: not followed")


def table_accesses(cls_name, plan, args, kwargs):
    """The byte intervals a table class's run() touches, from the pointers the object holds -> (reads, writes, unresolved)."""
    reads, writes, unresolved = [], [], []

    def add(group, path, t=None, ptr=None, nbytes=0):
        iv = (interval(t) if t.is_cuda else None) if t is not None else ((ptr, ptr + nbytes) if ptr and nbytes else None)
        if iv is not None:
            group.append((path, iv[0], iv[1]))
    if cls_name in ("AdamwPlan", "LambPlan"):
        for i in range(plan.n):
            x = plan.arr[i]
            for f in ("p", "m", "v"):
                add(writes, f"arr.{i}.{f}", ptr=getattr(x, f), nbytes=4 * x.n)
            add(reads, f"arr.{i}.g", ptr=x.g, nbytes=4 * x.n)
            add(writes, f"arr.{i}.pk", ptr=x.pk, nbytes=(4 if x.pk_f32 else 2) * x.n)
        for f in ("partials", "clip", "guard_state", "lamb_partials", "result"):
            if getattr(plan, f, None) is not None:
                add(writes, f, getattr(plan, f))
        if getattr(plan, "first_chunk", None) is not None:
            add(reads, "first_chunk", plan.first_chunk)
    elif cls_name == "AccumulatePlan":
        grads = args[0] if args else kwargs["grads"]
        for i in plan.live:
            add(writes, f"accs.{i}", plan.accs[i])
            add(reads, f"grads.{i}", grads[i])
    elif cls_name == "EmaPlan":
        for i, (s, p) in enumerate(plan.keep):
            add(writes, f"keep.{i}.0", s)
            add(reads, f"keep.{i}.1", p)
    elif cls_name == "PackPlan":
        add(reads, "table", plan.table)
        add(reads, "blk_start", plan.blk_start)
        for i, (it, tensors) in enumerate(zip(plan.items, plan.keep)):
            for j, t in enumerate(tensors):
                add(writes if t.data_ptr() in (it.out, it.bias_out) else reads, f"keep.{i}.{j}", t)
    elif cls_name == "TransposePlan":
        add(reads, "table", plan.table)
        add(reads, "blk_start", plan.blk_start)
        for i, (ptr, out) in enumerate(zip(plan.key, plan.outs)):
            add(reads, f"key.{i}", ptr=ptr, nbytes=out.numel() * 2)             # (dense source rows: the engine's packed weights)
            add(writes, f"outs.{i}", out)
    elif cls_name == "FoldPlan":
        for i, p in enumerate(plan.keep):
            add(reads, f"keep.{i}", p)
    else:
        unresolved.append(f"{cls_name}.run: a table whose pointers are not understood")
    return reads, writes, unresolved


class Recorder(contextlib.AbstractContextManager):
    """with Recorder() as rec: ... the step ...; afterwards rec.trace is the Trace.
    observe(name, [(path, tensor)]) -> callable or None: called around every TOP-LEVEL hip call (the write-table observation of
    tests/test_gpu_stream_order.py); the callable runs after the call."""

    def __init__(self, observe=None):
        self.trace, self.active, self.depth, self.observe, self._undo, self._quiet, self._keep = None, False, 0, observe, [], 0, []

    def _emit(self, fn, stream, reads, writes, unresolved=()):
        self.trace.events.append(("access", fn, stream, reads, writes, list(unresolved)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def traced(*a, **k):
            if not self.active:
                return fn(*a, **k)
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            tensors, unresolved = [], []
            for arg, v in bound.arguments.items():
                walk(v, arg, tensors, unresolved)
            stream = _raw_stream()
            if name in NO_TENSORS:
                if any(t.is_cuda for _, t in tensors):
                    self._emit(name, stream, [], [], [f"takes the tensor {tensors[0][0]} but is listed in NO_TENSORS"])
                return fn(*a, **k)
            if WRITES.get(name, ()) is None:                     # shapes only: no launch, no access
                return fn(*a, **k)
            after = self.observe(name, tensors) if self.observe is not None and self.depth == 0 else None
            self.depth += 1
            try:
                res = fn(*a, **k)
            finally:
                self.depth -= 1
            # noted when the call returns, with the stream it was entered on: its own temporaries and results exist by then (their
            # allocations are in the trace in front of it), and no binding records or waits for an event inside itself
            reads, writes, mine = [], [], set()
            for path, t in tensors:
                if not t.is_cuda or t.numel() == 0:
                    continue
                mine.add(interval(t))
                narrow = EXTENTS.get(name, {}).get(path)
                part = narrow(t, bound.arguments) if narrow is not None else None
                (writes if is_write(name, path) else reads).append((path, *interval(part if part is not None else t)))
            returned = []
            walk(res, RETURN, returned, [])
            for path, t in returned:
                if t.is_cuda and t.numel() and interval(t) not in mine:
                    if is_write(name, RETURN):
                        writes.append((path, *interval(t)))
                    else:
                        unresolved.append(f"hands back the tensor {path}, none of its arguments, and WRITES has no \"return\" for it")
            self._emit(name, stream, reads, writes, unresolved)
            if after is not None:
                after()
            return res
        return traced

    def _table_run(self, cls_name, fn):
        def traced(plan, *a, **k):
            if not self.active:
                return fn(plan, *a, **k)
            stream = _raw_stream()
            reads, writes, unresolved = table_accesses(cls_name, plan, a, k)
            results = []
            if cls_name == "FoldPlan":                           # the result buffer is allocated inside run(): seen through then()
                plan.then = [(off, N, (lambda r, then=then: (results.append(r), then(r))[1])) for off, N, then in plan.then]
            self.depth += 1
            try:
                res = fn(plan, *a, **k)
            finally:
                self.depth -= 1
            writes += [(f"result.{i}", *interval(r)) for i, r in enumerate(results)]
            self._emit(f"{cls_name}.run", stream, reads, writes, unresolved)
            return res
        return traced

    def _tables_init(self, fn):
        def traced(obj, cu, *a, **k):
            res = fn(obj, cu, *a, **k)
            if self.active:
                self._emit("QkvAttnTables", _raw_stream(), [("cu", *interval(cu))],
                           [(f, *interval(getattr(obj, f))) for f in ("rowseg", "tile_first", "ntiles")])
            return res
        return traced

    # ---- ATen
    def _dispatch_mode(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                kwargs = kwargs or {}
                if not rec.active:
                    return func(*args, **kwargs)
                events = rec.trace.events
                if func is torch.ops.aten.record_stream.default:
                    t = args[0]
                    if t.is_cuda and t.numel():
                        events.append(("record_stream", *_storage(t), _stream_handle(args[1])))
                    return func(*args, **kwargs)
                name, spec = str(func), func._schema.arguments
                ins = []                                         # (argument name, tensor, written)
                for sp, v in list(zip(spec, args)) + [(sp, kwargs[sp.name]) for sp in spec if sp.name in kwargs]:
                    w = sp.alias_info is not None and sp.alias_info.is_write
                    if isinstance(v, torch.Tensor):
                        ins.append((sp.name, v, w))
                    elif isinstance(v, (list, tuple)):
                        ins += [(f"{sp.name}.{i}", x, w) for i, x in enumerate(v) if isinstance(x, torch.Tensor)]
                out = func(*args, **kwargs)
                outs = [x for x in (out if isinstance(out, (list, tuple)) else (out,)) if isinstance(x, torch.Tensor)]
                have = {_storage(t)[0] for _, t, _ in ins if t.is_cuda}
                stream, fresh = _raw_stream(), []
                for i, t in enumerate(outs):
                    if t.is_cuda and t.numel() and _storage(t)[0] not in have:
                        have.add(_storage(t)[0])
                        fresh.append((f"out.{i}", t))
                        events.append(("alloc", stream, *_storage(t)))
                written = any(w for _, _, w in ins)
                view = bool(outs) and not fresh and not written and all(t.is_cuda for t in outs)     # every output aliases an input
                if not view:
                    reads = [(n, *interval(t)) for n, t, w in ins if t.is_cuda and t.numel() and not w]
                    writes = [(n, *interval(t)) for n, t, w in ins if t.is_cuda and t.numel() and w] + [(n, *interval(t)) for n, t in fresh]
                    if reads or writes:
                        events.append(("access", name, stream, reads, writes, []))
                    # the host waits for the current stream: .item(), and a copy to pageable / pinned host memory that is not
                    # asked to be non-blocking
                    to_host = any(not t.is_cuda for t in outs) or any(w and not t.is_cuda for _, t, w in ins)
                    non_blocking = kwargs.get("non_blocking", args[2] if "copy_" in name and len(args) > 2 else False)
                    if reads and ("_local_scalar_dense" in name or (to_host and not non_blocking)):
                        events.append(("sync", ("stream", stream)))
                return out
        return Mode()

    # ---- synchronisation calls
    def _patch(self, owner, attr, make):
        orig = getattr(owner, attr)
        setattr(owner, attr, make(orig))
        self._undo.append((owner, attr, orig))

    def _sync_calls(self):
        def log(*ev):
            if self.active and self._quiet == 0:
                self.trace.events.append(ev)

        def inner(fn, *a):                                       # (wait_stream records and waits for an event of its own: one entry)
            self._quiet += 1
            try:
                return fn(*a)
            finally:
                self._quiet -= 1

        def handle(stream):
            return _raw_stream() if stream is None else stream.cuda_stream

        def event_record(f):
            def record_(ev, stream=None):
                log("record", id(ev), handle(stream))
                self._keep.append(ev)
                return inner(f, ev, *(() if stream is None else (stream,)))
            return record_

        def event_wait(f):
            def wait_(ev, stream=None):
                log("wait_event", handle(stream), id(ev))
                return inner(f, ev, *(() if stream is None else (stream,)))
            return wait_

        def event_synchronize(f):
            def synchronize_(ev):
                log("sync", ("event", id(ev)))
                return inner(f, ev)
            return synchronize_

        def stream_wait_event(f):
            def wait_event_(st, ev):
                log("wait_event", st.cuda_stream, id(ev))
                return inner(f, st, ev)
            return wait_event_

        def stream_wait_stream(f):
            def wait_stream_(st, other):
                log("wait_stream", st.cuda_stream, other.cuda_stream)
                return inner(f, st, other)
            return wait_stream_

        def stream_record_event(f):
            def record_event_(st, event=None):
                ev = inner(f, st, *(() if event is None else (event,)))
                log("record", id(ev), st.cuda_stream)
                self._keep.append(ev)
                return ev
            return record_event_

        def stream_synchronize(f):
            def synchronize_(st):
                log("sync", ("stream", st.cuda_stream))
                return inner(f, st)
            return synchronize_

        def device_synchronize(f):
            def synchronize_(device=None):
                log("sync", None)
                return inner(f, device)
            return synchronize_
        E, S = torch.cuda.Event, torch.cuda.Stream
        for owner, attr, make in ((E, "record", event_record), (E, "wait", event_wait), (E, "synchronize", event_synchronize),
                                  (S, "wait_event", stream_wait_event), (S, "wait_stream", stream_wait_stream),
                                  (S, "record_event", stream_record_event), (S, "synchronize", stream_synchronize),
                                  (torch.cuda, "synchronize", device_synchronize)):
            self._patch(owner, attr, make)

    # ---- the context manager
    def __enter__(self):
        for name, fn in public_functions().items():
            self._patch(hip, name, lambda f, name=name: self._wrap(name, f))
        for cls in _TABLES:
            if "run" in vars(getattr(hip, cls)):
                self._patch(getattr(hip, cls), "run", lambda f, cls=cls: self._table_run(cls, f))
        self._patch(hip.QkvAttnTables, "__init__", self._tables_init)
        self._sync_calls()
        self._mode = self._dispatch_mode()
        self._mode.__enter__()
        self.trace = Trace(alive_start=_live_blocks(), main=_raw_stream())
        self.active = True
        return self

    def __exit__(self, *exc):
        self.active = False
        self._mode.__exit__(*exc)
        for owner, attr, orig in reversed(self._undo):
            setattr(owner, attr, orig)
        self._undo = []
        self.trace.alive_end = _live_blocks()
        return False

