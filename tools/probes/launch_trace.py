"""Launch trace of the forward paths: which msclip_amd.hip binding was called with which arguments, on which stream, in what order.

A host-side refactor of the engine changes no kernel, so "same behaviour" means "same launches with the same arguments".  This probe
wraps every public function of msclip_amd.hip (module attributes: the engine and train.py look them up at call time) and the two
cross-stream edges (Event.record, Stream.wait_event), runs a list of cases with the eager launch loop (plan=False: a replayed
table never enters Python) and writes one trace file per case plus digests.json (sha256 of the features and the loss).  A call is
one JSON line: the function, its arguments bound to the signature with defaults applied (so that a keyword left out and a keyword
given its default are the same launch), every tensor as [ordinal, dtype, shape, stride] -- the ordinal of its data_ptr() among the
distinct pointers of the case, which hides addresses and keeps aliasing and row offsets -- and the current stream's ordinal.

    python tools/probes/launch_trace.py OUT_DIR [case-name-substring ...]
    diff -r OUT_DIR_of_one_tree OUT_DIR_of_the_other

It imports msclip_amd only, so the same file runs against any checkout of the tree."""
import hashlib
import inspect
import json
import os
import sys

import torch

sys.path.insert(0, ".")
from msclip_amd import hip, options, synth, train                         # noqa: E402
from msclip_amd.config import named_config                                # noqa: E402
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model               # noqa: E402

B32, L14 = "b32-yfcc-msclips", "l14-fp8-msclips"


class Trace:
    def __init__(self):
        self.lines, self.ptrs, self.streams, self.events, self.depth, self.tensors = None, {}, {}, 0, 0, 0

    def start(self):
        self.lines, self.ptrs, self.streams, self.events = [], {}, {}, 0

    def stop(self):
        lines, self.lines = self.lines, None
        return lines

    def _ord(self, table, key):
        return table.setdefault(key, len(table))

    def stream(self, s=None):
        return self._ord(self.streams, (torch.cuda.current_stream() if s is None else s).cuda_stream)

    def value(self, v):
        if isinstance(v, torch.Tensor):
            self.tensors += 1
            return {"t": [self._ord(self.ptrs, v.data_ptr()), str(v.dtype), list(v.shape), list(v.stride())]}
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.value(x) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if type(v).__module__ == hip.__name__:              # FoldIn / FoldOut / QkvAttnTables: their fields
            return {type(v).__name__: self.value(vars(v))}
        return f"<{type(v).__name__}>"

    def call(self, name, args):
        self.lines.append(json.dumps({"fn": name, "stream": self.stream(), "args": args}))

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def traced(*a, **k):
            if self.lines is not None and self.depth == 0:       # (a binding that calls another one is one entry)
                bound = sig.bind(*a, **k)
                bound.apply_defaults()
                self.tensors = 0
                args = self.value(dict(bound.arguments))
                if self.tensors:                                  # takes tensors: a launch (or a table built from tensors)
                    self.call(name, args)
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
        return traced

    def install(self):
        for name, fn in list(vars(hip).items()):
            if inspect.isfunction(fn) and fn.__module__ == hip.__name__ and not name.startswith("_"):
                setattr(hip, name, self.wrap(name, fn))
        record, wait = torch.cuda.Event.record, torch.cuda.Stream.wait_event

        def traced_record(ev, stream=None):
            if self.lines is not None:
                ev._trace_id, self.events = self.events, self.events + 1
                self.lines.append(json.dumps({"fn": "event.record", "event": ev._trace_id, "stream": self.stream(stream)}))
            return record(ev) if stream is None else record(ev, stream)

        def traced_wait(stream, ev):
            if self.lines is not None:
                self.lines.append(json.dumps({"fn": "stream.wait_event", "event": getattr(ev, "_trace_id", -1),
                                              "stream": self.stream(stream)}))
            return wait(stream, ev)
        torch.cuda.Event.record, torch.cuda.Stream.wait_event = traced_record, traced_wait


TRACE = Trace()
_MODELS = {}


def model(name, precision=None, fresh=False):
    key = (name, precision)
    if fresh or key not in _MODELS:
        m = get_clip_model(named_config(name, ["MODEL.SPEC.PRECISION", precision] if precision else None))
        m.load_state_dict(synth.synth_state_dict(synth.schema_of(m)), strict=True)
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


def digest(t):
    return hashlib.sha256(t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def inputs(B, _cache={}):
    if B not in _cache:
        _cache[B] = synth.synth_images(B, seed=51).cuda(), synth.synth_tokens(B, seed=52).cuda()
    return _cache[B]


def engine_case(name, B, call="run", precision=None, calibrate=None, fresh=False, **opt):
    """calibrate: True = calibrate_fp8 first, False = never (single-tower calls of an fp8 engine), None = whatever run() does."""
    def go():
        eng = model(name, precision, fresh).engine()
        taps = opt.pop("taps", None)
        eng.opt = type(eng.opt)().replace(plan=False, **opt)
        img, tok = inputs(B)
        if calibrate:
            eng.calibrate_fp8(img, tok)
        elif calibrate is False:
            eng._fp8_warned = True
        fold, eligible = [], type(eng)._fold_eligible.__get__(eng)      # what each _blocks call of the traced run decided

        def noted(*a):
            fold.append(eligible(*a))
            return fold[-1]
        eng.__dict__["_fold_eligible"] = noted

        def once():
            del fold[:]
            if call == "run":
                ws = eng.run(img, tok, taps={} if taps else None)
                return {"fv": ws["fv"], "ft": ws["ft"]}
            if call == "calibrate_fp8":
                eng.calibrate_fp8(img, tok)
                ws = eng.run(img, tok)
                return {"fv": ws["fv"], "ft": ws["ft"]}
            if call == "encode_image":
                return {"fv": eng.encode_image(img)}
            if call == "encode_text":
                return {"ft": eng.encode_text(tok)}
            if call == "forward_logits":
                return {"logits": eng.forward_logits(img, tok, gather=False)}
            return {"loss": eng.forward_loss(img, tok, gather=False)}
        return once, lambda: dict(fold_eligible=list(fold), dynamic_rows=eng.dynamic_rows(B, B))
    return go


def train_case(B, compact=True, masks=False):
    def go():
        m = model(B32, None)
        ts = train.TrainStep(m, lr=1e-4, bn="frozen")
        m.engine().opt = type(m.engine().opt)().replace(plan=False)
        img, tok = inputs(B)
        dm = None
        if masks:
            g = torch.Generator().manual_seed(7)
            dm = torch.rand(ts.drop_mask_shape(B), generator=g) < 0.8
        saved = options.TRAIN

        def once():
            options.TRAIN = saved.replace(compact_last_block=compact)
            try:
                loss = ts.forward(img, tok, drop_masks=dm)
            finally:
                options.TRAIN = saved
            return {"loss": loss, "fv": ts.saved["fv"], "ft": ts.saved["ft"]}
        return once, dict
    return go


def cases():
    out = {}
    for prec, tag, kw in (("bf16", "bf16", {}), ("fp8", "fp8cal", dict(calibrate=True)), ("fp8-qkv", "fp8qkv", dict(calibrate=True))):
        for B in (4, 256):
            for call in ("run", "encode_image", "encode_text", "forward_loss"):
                out[f"{tag}_b{B}_{call}"] = engine_case(B32, B, call, prec, **kw)
    for B in (4, 256):
        # fp8 without a calibration run: the single-tower calls of a fresh engine, then the calibration pass itself
        out[f"fp8nocal_b{B}_encode_image"] = engine_case(B32, B, "encode_image", "fp8", calibrate=False, fresh=True)
        out[f"fp8nocal_b{B}_encode_text"] = engine_case(B32, B, "encode_text", "fp8", calibrate=False, fresh=True)
        out[f"fp8_b{B}_calibrate_fp8"] = engine_case(B32, B, "calibrate_fp8", "fp8")
        out[f"bf16_b{B}_forward_logits"] = engine_case(B32, B, "forward_logits", "bf16")
        for opt in (dict(ln_fold=False), dict(text_pack=False), dict(dynamic_rows=False), dict(full_last_block=True),
                    dict(last_block_all_queries=True), dict(adapter_ln1_pass=True), dict(fused_qkv_attn=True),
                    dict(conv_side_stream=False), dict(text0_stream=False), dict(taps=True)):
            (k, v), = opt.items()
            out[f"bf16_b{B}_run_{k}={int(v)}"] = engine_case(B32, B, "run", "bf16", **opt)
        out[f"fp8cal_b{B}_run_last_block_all_queries=1"] = engine_case(B32, B, "run", "fp8", calibrate=True, last_block_all_queries=True)
    # the patch-stem model (no conv stem, no adapters: two segments from layer 0 on, separate weights there) and the 14 x 14 grid
    for call in ("run", "encode_image", "encode_text", "forward_loss"):
        out[f"l14_bf16_b4_{call}"] = engine_case(L14, 4, call, "bf16")
    out["l14_bf16_b256_run"] = engine_case(L14, 256, "run", "bf16")
    out["l14_fp8cal_b4_run"] = engine_case(L14, 4, "run", "fp8", calibrate=True)
    out["l14_fp8cal_b256_run"] = engine_case(L14, 256, "run", "fp8", calibrate=True)
    out["b16_bf16_b256_run"] = engine_case("b16-yfcc-msclips", 256)
    out["b16_bf16_b256_run_taps=1"] = engine_case("b16-yfcc-msclips", 256, taps=True)
    out["train_b8_compact"] = train_case(8)
    out["train_b8_full_last_block"] = train_case(8, compact=False)
    out["train_b8_drop_masks"] = train_case(8, masks=True)
    return out


def main():
    out_dir, want = sys.argv[1], sys.argv[2:]
    os.makedirs(out_dir, exist_ok=True)
    TRACE.install()
    summary = {}
    for name, make in cases().items():
        if want and not any(s in name for s in want):
            continue
        once, info = make()
        once()                                                   # warm-up: workspaces, weight caches, lazy tables
        torch.cuda.synchronize()
        TRACE.start()
        res = once()
        lines = TRACE.stop()
        torch.cuda.synchronize()
        with open(os.path.join(out_dir, name + ".trace"), "w") as f:
            f.write("\n".join(lines) + "\n")
        summary[name] = dict(lines=len(lines), sha256={k: digest(v) for k, v in res.items()}, **info())
        print(name, len(lines), flush=True)
    with open(os.path.join(out_dir, "digests.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
