"""Cost of the LAMB optimizer phase (TRAIN.OPTIMIZER lamb) against AdamW's on one MI355X, in one process on one GPU:

    python tools/probes/lamb_bench.py [--model b32-yfcc-msclips] [--rounds 24] [--calls 20] [--out profiles/lamb_optimizer_phase.json]

Twin models, TrainStep(optimizer="adamw") and TrainStep(optimizer="lamb"), one backward's gradients; after a warm-up step each,
the optimizer tables' run() -- the whole phase: one msclip_adamw_multi call, or msclip_lamb_partials -> msclip_lamb_ratios ->
msclip_lamb_apply; with --clip also the two calls of the clip norm in front of either -- is timed with HIP events around
windows of --calls back-to-back runs, the arms alternating, --rounds windows each after one warm-up round.  The three LAMB calls
are then timed one by one the same way.

What the ratio should approach is the bytes moved per element: AdamW reads p, g, m, v and writes p, m, v (28 B; the packed
copies add 2 B on the projection tensors of both arms); LAMB reads p, g, m, v once more in front of it (16 B): 44 / 28 = 1.57,
with the clip norm's 4 B in front of both 48 / 32 = 1.50."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls               # us per call


def _alternate(arms, rounds, calls):
    win = {k: [] for k in arms}
    for r in range(rounds + 1):
        for name, fn in arms.items():
            us = _window(fn, calls)
            if r:
                win[name].append(us)
    return win


def _stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "windows": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=16, help="batch of the one backward that supplies the gradients")
    ap.add_argument("--rounds", type=int, default=24, help="timed windows per arm")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back optimizer phases per window")
    ap.add_argument("--out", default="", help="write the figures to this JSON file")
    args = ap.parse_args()
    from msclip_amd import hip, synth, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    from bench import load_schema
    dev = torch.device("cuda", 0)
    cfg = named_config(args.model, ["MODEL.SPEC.PRECISION", "bf16"])

    def fresh():
        m = get_clip_model(cfg)
        m.load_state_dict(synth.synth_state_dict(load_schema(args.model), seed=0), strict=True)
        return m.to(dev).eval()
    twins = {"adamw": train.TrainStep(fresh(), lr=1e-4, bn="frozen"),
             "lamb": train.TrainStep(fresh(), lr=1e-3, bn="frozen", optimizer="lamb")}
    ts = twins["adamw"]
    ts.forward(synth.synth_images(args.batch, seed=10).to(dev), synth.synth_tokens(args.batch, seed=100).to(dev))
    grads = ts.backward(clone=True)
    ts.saved = None
    n = sum(g.numel() for g in grads.values())
    norm = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))
    plans = {}
    for name, t in twins.items():
        t.step(grads)                                      # warm-up: builds the table, loads the code objects
        plans[name] = t._adamw_plan(grads)
    b1, b2 = ts.betas
    result = {"model": args.model, "parameter_tensors": len(grads), "elements": n, "table_items": {k: p.n for k, p in plans.items()},
              "rounds": args.rounds, "calls_per_window": args.calls, "device": torch.cuda.get_device_name(0)}
    for clip in (None, 0.5 * norm):
        tag = "clipped" if clip else "unclipped"
        arms = {"adamw": lambda: plans["adamw"].run(b1, b2, 1e-8, 2, clip), "lamb": lambda: plans["lamb"].run(b1, b2, 1e-6, 2, clip)}
        win = _alternate(arms, args.rounds, args.calls)
        a, l = statistics.median(win["adamw"]), statistics.median(win["lamb"])
        bytes_a, bytes_l = (32, 48) if clip else (28, 44)
        result[tag] = {"adamw": _stats(win["adamw"]), "lamb": _stats(win["lamb"]), "lamb_over_adamw": l / a,
                       "byte_ratio": bytes_l / bytes_a, "adamw_TBps": bytes_a * n / a / 1e6, "lamb_TBps": bytes_l * n / l / 1e6}
        print(f"{tag}: AdamW phase {a:.1f} us ({bytes_a * n / a / 1e6:.2f} TB/s), LAMB phase {l:.1f} us ({bytes_l * n / l / 1e6:.2f} TB/s), "
              f"ratio {l / a:.3f} (bytes {bytes_l}/{bytes_a} = {bytes_l / bytes_a:.3f})")
    # the three LAMB calls one by one
    p, L = plans["lamb"], hip.lib()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)     # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    calls = {
        "msclip_lamb_partials": lambda: L.msclip_lamb_partials(p.arr, p.n, b1, b2, 1e-6, 2, None, ptr(p.lamb_partials), 2 * p.n_chunks, st()),
        "msclip_lamb_ratios": lambda: L.msclip_lamb_ratios(ptr(p.lamb_partials), ptr(p.first_chunk), p.n_params, p.n_chunks, 0, ptr(p.result), st()),
        "msclip_lamb_apply": lambda: L.msclip_lamb_apply(p.arr, p.n, b1, b2, 1e-6, 2, None, ptr(p.result), st()),
        "msclip_adamw_multi": lambda: L.msclip_adamw_multi(plans["adamw"].arr, plans["adamw"].n, b1, b2, 1e-8, 2, st()),
    }
    win = _alternate(calls, args.rounds, args.calls)
    result["per_call"] = {k: _stats(v) for k, v in win.items()}
    for k, v in win.items():
        print(f"  {k:<22s} median {statistics.median(v):8.1f} us   min {min(v):8.1f}   max {max(v):8.1f}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
