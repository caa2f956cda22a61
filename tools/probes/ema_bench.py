"""Cost of the weight EMA (TRAIN.EMA_DECAY) on one MI355X, two measurements in one process on one GPU:

    python tools/probes/ema_bench.py [--model b32-yfcc-msclips] [--batch 512] [--rounds 20] [--calls 50] [--pairs 12]

1. The launch alone.  One msclip_ema_multi call over the model's parameter list (shadow arena as TrainStep lays it out)
   against one msclip_grad_accumulate call in mode 1 (acc += g) over the same list, accumulators laid out like the shadows and
   the parameters as `g`: both move 12 B per element with the same access pattern, so the accumulate kernel is the
   yardstick; the EMA has two more multiplies per element.  HIP events around windows of --calls back-to-back calls, the two
   arms alternating, --rounds windows each after one warm-up round; the spread of the windows is printed with the medians.
2. The training step.  Twin models, TrainStep without and with ema_decay, frozen BatchNorm, alternating whole steps
   (forward + backward + step, HIP events, a synchronise between steps), --pairs timed pairs after two warm-up pairs; also
   the optimizer phase (events around step()) on its own.

Floor of the launch: 12 B x parameter count at what a streaming read-modify-write reaches on this chip."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out                  # us


def _line(name, xs):
    med = statistics.median(xs)
    return f"  {name:<22s} median {med:9.1f} us   min {min(xs):9.1f}   max {max(xs):9.1f}   spread {100 * (max(xs) - min(xs)) / med:4.1f} %"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=20, help="timed windows per arm of the kernel measurement")
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per window")
    ap.add_argument("--pairs", type=int, default=12, help="timed (EMA off, EMA on) step pairs after two warm-up pairs; 0 = skip")
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
    model = fresh()
    # ---- 1. the launch alone
    ema = train._EmaShadow(model)
    params = [p.data.view(-1) for p in ema.params.values()]
    acc = train._EmaShadow(model)                          # a second arena of the same layout: the yardstick's accumulators
    aplan = hip.AccumulatePlan([v.view(-1) for v in acc.views.values()])
    acc.arena.zero_()
    n = sum(p.numel() for p in params)
    arms = {"msclip_ema_multi": lambda: ema.plan.run(0.999), "msclip_grad_accumulate": lambda: aplan.run(params, 1)}
    win = {k: [] for k in arms}
    for r in range(args.rounds + 1):
        for name, fn in arms.items():
            us, _ = _timed(lambda: [fn() for _ in range(args.calls)])
            if r:
                win[name].append(us / args.calls)
    e, a = statistics.median(win["msclip_ema_multi"]), statistics.median(win["msclip_grad_accumulate"])
    print(f"{args.model}: {len(params)} parameter tensors, {n} elements, 12 B x elements = {12 * n / 1e6:.1f} MB per call")
    print(f"per call, {args.rounds} alternating windows of {args.calls} back-to-back calls (HIP events):")
    for name in arms:
        print(_line(name, win[name]) + f"   {12 * n / statistics.median(win[name]) / 1e6:.2f} TB/s")
    print(f"  EMA / accumulate = {e / a:.3f} (expected within 1.10)")
    del ema, acc, aplan, arms
    if args.pairs <= 0:
        return
    # ---- 2. the training step
    twins = {"off": train.TrainStep(model, lr=1e-4, bn="frozen"), "on": train.TrainStep(fresh(), lr=1e-4, bn="frozen", ema_decay=0.999)}
    img, tok = synth.synth_images(args.batch, seed=10).to(dev), synth.synth_tokens(args.batch, seed=100).to(dev)
    whole, opt = {k: [] for k in twins}, {k: [] for k in twins}

    def step(ts):
        ts.forward(img, tok)
        grads = ts.backward()
        return _timed(lambda: ts.step(grads))[0]
    for i in range(args.pairs + 2):
        for arm, ts in twins.items():
            torch.cuda.synchronize()
            us, us_opt = _timed(lambda: step(ts))
            if i >= 2:
                whole[arm].append(us)
                opt[arm].append(us_opt)
    print(f"training step, batch {args.batch}, bn=frozen, {args.pairs} alternating pairs (HIP events):")
    for arm in twins:
        print(_line(f"step, EMA {arm}", whole[arm]))
    for arm in twins:
        print(_line(f"step() alone, EMA {arm}", opt[arm]))
    d_whole = statistics.median(whole["on"]) - statistics.median(whole["off"])
    d_opt = statistics.median(opt["on"]) - statistics.median(opt["off"])
    print(f"  extra with EMA on: {d_whole:.1f} us of the step ({100 * d_whole / statistics.median(whole['off']):.2f} %), "
          f"{d_opt:.1f} us of step() alone; EMA updates {twins['on'].ema_updates}")


if __name__ == "__main__":
    main()
