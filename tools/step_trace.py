"""What one training step issues, in a form two commits can be diffed by (a restructuring of TrainStep.forward / backward must
leave every part equal):

    python tools/step_trace.py --out step_trace.json [--cases frozen batch ...]

Per case: forward() + backward() (accumulate() in its case) on its SECOND call, after a warm-up that allocates workspaces and
lazy tables, under tests/stream_order.Recorder, as tests/test_gpu_stream_order.py::_traced does.  No optimizer step: the token
embedding's gradient is an atomic scatter-add, and an update from it would make the traced call's weights differ from run to
run.  The "reweighted" kind halves every conv-side parameter in place between the warm-up and the traced call instead (exact, and
the engine repacks): a transposed or packed operand that outlives its weights shows in the hashes.  Synthetic weights and
inputs, fixed seeds, plan=False.  One JSON file, per case:
  "order"   the issue-order record: every access as [name, stream role, reads, writes] with reads / writes as [argument, bytes],
            every alloc / record_stream / record / wait_event / wait_stream / sync in place; streams and events as indices by
            first appearance, sizes instead of addresses;
  "counts"  Trace.counts() and the number of events;
  "sha256"  of the loss's bytes and of every returned gradient's bytes, by key;
  "buffers" (bn="batch" only) sha256 of every BatchNorm running_mean / running_var / num_batches_tracked after the traced call;
  "peak"    torch.cuda.max_memory_allocated() of the traced call; "peak_above_base": less what was allocated when it began.
GPU only; reads nothing outside the repository; not a test."""
import argparse
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402
import stream_order as so                                # noqa: E402
from msclip_amd import options, synth, train             # noqa: E402
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model      # noqa: E402
from msclip_amd.config import named_config               # noqa: E402

B32, B16, L14 = "b32-yfcc-msclips", "b16-yfcc-msclips", "l14-fp8-msclips"
#        name: (model, extra config, TrainStep bn, batch, EngineOptions fields, TrainOptions fields, kind)
CASES = {"frozen": (B32, [], "frozen", 4, {}, {}, "step"),
         "batch": (B32, [], "batch", 4, {}, {}, "step"),
         "droppath": (B32, ["MODEL.SPEC.VISION.DROP_PATH", "0.2"], "frozen", 4, {}, {}, "masks"),
         "full_last_block": (B32, [], "frozen", 4, {}, dict(compact_last_block=False), "step"),
         "accumulate": (B32, [], "frozen", 4, {}, {}, "accumulate"),
         "l14": (L14, [], "frozen", 4, {}, {}, "step"),
         "rows256": (B32, [], "frozen", 256, dict(text_pack=False), {}, "step"),
         "wgrad_sync": (B32, [], "frozen", 4, {}, dict(wgrad_sync=True), "step"),
         # the conv side (train_conv.py) beyond its defaults: every fallback of the train-mode walk, the column-matrix / main-stream
         # forms of the frozen one, no lane, the other map sizes (parity-plan thresholds), chunks, weights that changed
         "batch_plain": (B32, [], "batch", 4, {},
                         dict(bn_two_pass=False, bn_bwd_fused=False, adapter_bn_views=False, raw_pack_table=False), "step"),
         "frozen_col2im": (B32, [], "frozen", 4, {}, dict(dgrad_col2im=True, im2col_main=True, colsum_main=True), "step"),
         "batch_wgrad_sync": (B32, [], "batch", 4, {}, dict(wgrad_sync=True), "step"),
         "b16_frozen": (B16, [], "frozen", 4, {}, {}, "step"),
         "b16_batch": (B16, [], "batch", 4, {}, {}, "step"),
         "batch_accumulate": (B32, [], "batch", 4, {}, {}, "accumulate"),
         "frozen_reweighted": (B32, [], "frozen", 4, {}, {}, "reweighted"),
         "batch_reweighted": (B32, [], "batch", 4, {}, {}, "reweighted")}
CONV_SIDE = ("visual.transformer.resblocks.0.", "visual.transformer.parallel_branch_v.", "visual.transformer.parallel_lateral_adapter.")
BN_BUFFERS = (".running_mean", ".running_var", ".num_batches_tracked")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def order(trace):
    """The trace's events with handles and addresses replaced by what survives a rerun."""
    streams, events = {}, {}

    def role(s):
        return streams.setdefault(s, len(streams))

    def ev(x):
        return events.setdefault(x, len(events))

    def sizes(group):
        return [[name, hi - lo] for name, lo, hi in group]
    out = []
    for e in trace.events:
        kind = e[0]
        if kind == "access":
            out.append([kind, e[1], role(e[2]), sizes(e[3]), sizes(e[4])])
        elif kind == "alloc":
            out.append([kind, role(e[1]), e[3] - e[2]])
        elif kind == "record_stream":
            out.append([kind, e[2] - e[1], role(e[3])])
        elif kind == "record":
            out.append([kind, ev(e[1]), role(e[2])])
        elif kind == "wait_event":
            out.append([kind, role(e[1]), ev(e[2])])
        elif kind == "wait_stream":
            out.append([kind, role(e[1]), role(e[2])])
        else:                                            # sync: None / ("stream", s) / ("event", e)
            what = e[1]
            out.append([kind, None if what is None else [what[0], role(what[1]) if what[0] == "stream" else ev(what[1])]])
    return out


def run_case(name):
    model_name, extra, bn, B, eng_opt, train_opt, kind = CASES[name]
    gc.collect()                                         # (the previous case's model: its engine holds it in a cycle)
    torch.cuda.empty_cache()
    with open(os.path.join(ROOT, "tests", "golden", model_name + ".schema.json")) as f:
        schema = [(k, tuple(s), getattr(torch, d)) for k, s, d in json.load(f)]
    m = get_clip_model(named_config(model_name, ["MODEL.SPEC.PRECISION", "bf16"] + extra))
    m.load_state_dict(synth.synth_state_dict(schema, seed=0), strict=True)
    m = m.cuda().eval()
    eng = m.engine()
    eng.opt = eng.opt.replace(plan=False, **eng_opt)
    kept, options.TRAIN = options.TRAIN, options.TRAIN.replace(**train_opt)
    try:
        ts = train.TrainStep(m, lr=1e-4, bn=bn)
        n = 2 * B if kind == "accumulate" else B
        img, tok = synth.synth_images(n, seed=51).cuda(), synth.synth_tokens(n, seed=52).cuda()
        masks = None
        if kind == "masks":
            gen = torch.Generator(device="cuda").manual_seed(7)
            masks = torch.rand(ts.drop_mask_shape(B), generator=gen, device="cuda") < 0.8

        def once():
            if kind == "accumulate":
                return ts.accumulate([(img[:B], tok[:B]), (img[B:], tok[B:])])
            loss = ts.forward(img, tok, drop_masks=masks)
            return loss, ts.backward()
        once()
        if kind == "reweighted":
            with torch.no_grad():
                for k, p in m.named_parameters():
                    if k.startswith(CONV_SIDE):
                        p.mul_(0.5)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with so.Recorder() as rec:
            loss, grads = once()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
    finally:
        options.TRAIN = kept
    hashes = {"loss": sha(loss)}
    hashes.update({k: sha(g) for k, g in sorted(grads.items())})
    rec_order = order(rec.trace)
    out = dict(order=rec_order, counts=dict(rec.trace.counts(), records=len(rec_order)), sha256=hashes, peak=peak,
               peak_above_base=peak - base)
    if bn == "batch":
        out["buffers"] = {k: sha(b) for k, b in sorted(m.named_buffers()) if k.endswith(BN_BUFFERS)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    args = ap.parse_args()
    result = {}
    for name in args.cases:
        result[name] = run_case(name)
        print(name, result[name]["counts"], "peak", result[name]["peak"], flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=0)


if __name__ == "__main__":
    main()
