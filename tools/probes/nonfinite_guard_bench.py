"""Cost of the non-finite guard (TrainStep(nonfinite="skip")) inside the optimizer phase and on the whole step: the method of
tools/probes/clip_grad_bench.py -- HIP events around TrainStep.step() on the ViT-B/32 batch-512 training step, the arms
alternating step by step in one process on one GPU -- plus chains of steps issued back to back without a synchronisation, which
is where the guard's one-step cap on the host's lead would show.

    python tools/probes/nonfinite_guard_bench.py [--model b32-yfcc-msclips] [--batch 512] [--rounds 10] [--chain 6] [--bn batch]
                                                 [--arms plain,guard,clip,clip+guard]

Arms: plain (no clipping, no guard), guard, clip (max_norm far above the norm: coef = 1, the same trajectory), clip+guard.  No
gradient here is non-finite, so no step is skipped and all arms walk one trajectory.  --arms plain,clip runs on a commit that
has no guard (for the comparison with the parent commit)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402

ARMS = {"plain": (None, None), "guard": ("skip", None), "clip": (None, 1e30), "clip+guard": ("skip", 1e30)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=10, help="timed rounds over the arms after two warm-up rounds")
    ap.add_argument("--chain", type=int, default=6, help="steps per back-to-back chain (0: no chains)")
    ap.add_argument("--bn", choices=("batch", "frozen"), default="batch")
    ap.add_argument("--arms", default="plain,guard,clip,clip+guard")
    args = ap.parse_args()
    arms = args.arms.split(",")
    assert all(a in ARMS for a in arms), arms
    from msclip_amd import synth, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    from bench import load_schema
    dev = torch.device("cuda", 0)
    cfg = named_config(args.model, ["MODEL.SPEC.PRECISION", "bf16"])
    model = get_clip_model(cfg)
    model.load_state_dict(synth.synth_state_dict(load_schema(args.model), seed=0), strict=True)
    model = model.to(dev).eval()
    ts = train.from_config(model, cfg, bn=args.bn)
    img, tok = synth.synth_images(args.batch, seed=10).to(dev), synth.synth_tokens(args.batch, seed=100).to(dev)

    def select(arm):
        guard, max_norm = ARMS[arm]
        if guard is not None or hasattr(ts, "nonfinite"):
            ts.nonfinite = guard
        ts.clip_grad_norm = max_norm

    phase = {a: [] for a in arms}
    whole = {a: [] for a in arms}
    for r in range(args.rounds + 2):
        for arm in (arms if r % 2 == 0 else arms[::-1]):   # (the order flips every round: no arm always follows the same one)
            select(arm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ts.forward(img, tok)
            grads = ts.backward()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ts.step(grads)
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del grads
            if r >= 2:
                phase[arm].append(a.elapsed_time(b) * 1e3)
                whole[arm].append((t1 - t0) * 1e3)
    chains = {a: [] for a in arms}
    if args.chain > 0:
        for r in range(args.rounds // 2 + 1):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                select(arm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.chain):                # back to back: the host runs ahead as far as the step lets it
                    ts.forward(img, tok)
                    ts.step(ts.backward())
                torch.cuda.synchronize()
                if r >= 1:
                    chains[arm].append((time.perf_counter() - t0) * 1e3 / args.chain)
    plan = ts._plan
    nparam = sum(plan.arr[i].n for i in range(plan.n))
    print(f"{args.model} batch {args.batch} bn={args.bn}: {plan.n} table entries, {nparam} elements "
          f"({4 * nparam / 1e6:.1f} MB of gradients), {plan.n_partials} partials; {args.rounds} rounds, arms alternating")
    print("optimizer phase, HIP events around step() [us]: median (min .. max)")
    for arm in arms:
        t = phase[arm]
        print(f"  {arm:11s} {statistics.median(t):9.1f}  ({min(t):.1f} .. {max(t):.1f})")
    print("forward + backward + step with a synchronisation in front of step() and behind it, wall clock [ms]: median (min .. max)")
    for arm in arms:
        t = whole[arm]
        print(f"  {arm:11s} {statistics.median(t):9.2f}  ({min(t):.2f} .. {max(t):.2f})")
    if args.chain > 0:
        print(f"chains of {args.chain} steps issued back to back, one synchronisation at the end, wall clock per step [ms]: median (min .. max)")
        for arm in arms:
            t = chains[arm]
            print(f"  {arm:11s} {statistics.median(t):9.2f}  ({min(t):.2f} .. {max(t):.2f})")
    med = {a: statistics.median(phase[a]) for a in arms}
    if "plain" in med and "guard" in med:
        d = med["guard"] - med["plain"]
        print(f"guard alone - plain: {d:.1f} us = {100 * d / med['plain']:.1f} % of the phase; 4 B x elements / extra = "
              f"{4 * nparam / max(d, 1e-9) / 1e6:.2f} TB/s")
    if "clip" in med and "clip+guard" in med:
        d = med["clip+guard"] - med["clip"]
        print(f"clip + guard - clip: {d:.1f} us = {100 * d / med['clip']:.2f} % of the phase")
    if getattr(ts, "nonfinite", None) is not None or "guard" in arms:
        ts.nonfinite = "skip"
        print(f"skipped steps: {ts.skipped_steps} of {ts.steps}")


if __name__ == "__main__":
    main()
