"""Cost of gradient clipping inside the optimizer phase: HIP events around TrainStep.step() on the
ViT-B/32 batch-512 training step, alternating unclipped / clipped steps in one process on one GPU.

    python tools/probes/clip_grad_bench.py [--model b32-yfcc-msclips] [--batch 512] [--pairs 12] [--bn batch]

The clipped arm runs with a max_norm far above the norm, so coef = 1 and both arms walk the same trajectory (the clipped
kernel multiplies by the coefficient either way).  Floor of the extra cost: one more read of the gradients, 4 bytes x
parameter count at what a streaming read reaches (about 6 TB/s on this chip), plus two launch boundaries.  Also timed on
their own: the two norm calls (msclip_grad_sumsq + msclip_clip_coef) on the step's gradient table."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=12, help="timed (unclipped, clipped) step pairs after two warm-up pairs")
    ap.add_argument("--bn", choices=("batch", "frozen"), default="batch")
    args = ap.parse_args()
    from msclip_amd import hip, synth, train
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
    times = {"off": [], "on": []}
    norm_only = []
    for i in range(2 * (args.pairs + 2)):
        arm = "on" if i % 2 else "off"
        ts.clip_grad_norm = 1e30 if arm == "on" else None
        ts.forward(img, tok)
        grads = ts.backward()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ts.step(grads)
        b.record()
        torch.cuda.synchronize()
        if i >= 4:
            times[arm].append(a.elapsed_time(b) * 1e3)
        if arm == "on" and i >= 4:                         # the two norm calls alone, on the table the step has just used
            p = ts._plan
            L, st = hip.lib(), hip._stream()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hip._check(L.msclip_grad_sumsq(p.sq, p.n_sq, hip._p(p.partials), p.n_partials, st), "msclip_grad_sumsq")
            hip._check(L.msclip_clip_coef(hip._p(p.partials), p.n_partials, 1e30, hip._p(p.clip), st), "msclip_clip_coef")
            b.record()
            torch.cuda.synchronize()
            norm_only.append(a.elapsed_time(b) * 1e3)
        del grads
    nparam = sum(ts._plan.arr[i].n for i in range(ts._plan.n))
    off, on, alone = (statistics.median(times["off"]), statistics.median(times["on"]), statistics.median(norm_only))
    print(f"{args.model} batch {args.batch} bn={args.bn}: {ts._plan.n} table entries, {ts._plan.n_sq} gradient tensors, "
          f"{nparam} elements ({4 * nparam / 1e6:.1f} MB of gradients), {ts._plan.n_partials} partials")
    print(f"optimizer phase (events around step()), median of {len(times['off'])} alternating pairs:")
    print(f"  unclipped {off:9.1f} us   (min {min(times['off']):.1f}, max {max(times['off']):.1f})")
    print(f"  clipped   {on:9.1f} us   (min {min(times['on']):.1f}, max {max(times['on']):.1f})")
    print(f"  extra     {on - off:9.1f} us = {100 * (on - off) / off:.1f} % of the phase; 4 B x elements / extra = "
          f"{4 * nparam / max(on - off, 1e-9) / 1e6:.2f} TB/s")
    print(f"norm calls alone (sumsq launches + fold): median {alone:.1f} us (min {min(norm_only):.1f}) = "
          f"{4 * nparam / alone / 1e6:.2f} TB/s of gradient bytes")
    print(f"grad norm of the last clipped step: {ts.last_grad_norm.item():.6g}, coef {ts.last_clip_coef.item():.6g}")


if __name__ == "__main__":
    main()
