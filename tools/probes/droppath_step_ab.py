"""Training-step time and launch counts with stochastic depth off / on, one arm per process on one MI355X:

    python tools/probes/droppath_step_ab.py [--tree DIR] [--bn frozen|batch] [--drop-path P] [--mode sample|position]
                                            [--model b32-yfcc-msclips] [--batch 512] [--steps 20] [--warmup 5]

One process = one arm: --tree names the checkout whose msclip_amd is imported (default: this one; a checkout of the parent
commit, built, for the "parent" arm -- there --drop-path must stay 0), so that a shell loop can alternate parent / off / on
on the same box.  Whole steps (forward + backward + step on one fixed batch, captions staged a step ahead as bench.py does),
HIP events per step with a synchronise between steps; prints one JSON line: median / min / max step time and, for ONE step, the
calls into libmsclip_hip.so by entry point (a counting proxy in front of the ctypes library: every kernel launch of the
library is one call) -- the off arm must show the parent's counts, the on arm the same total with msclip_gemm_rowscale /
msclip_layernorm_bwd_rowscale / msclip_cast_bf16_colsum_rowscale in place of their plain forms."""
import argparse
import collections
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--arm", default="")
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--bn", choices=("frozen", "batch"), default="frozen")
    ap.add_argument("--drop-path", type=float, default=0.0)
    ap.add_argument("--mode", default="sample")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import msclip_amd
    msclip_amd.configure_runtime()
    import torch
    from msclip_amd import hip, synth, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    from bench import load_schema
    assert os.path.abspath(msclip_amd.__file__).startswith(os.path.abspath(args.tree)), msclip_amd.__file__
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = named_config(args.model, ["MODEL.SPEC.PRECISION", "bf16"])
    model = get_clip_model(cfg)
    model.load_state_dict(synth.synth_state_dict(load_schema(args.model), seed=0), strict=True)
    model = model.to(dev).eval()
    kw = dict(drop_path=args.drop_path, drop_path_mode=args.mode) if args.drop_path else {}
    ts = train.TrainStep(model, bn=args.bn, **train.optimizer_settings(cfg), **kw)
    img, tok = synth.synth_images(args.batch, seed=10).to(dev), synth.synth_tokens(args.batch, seed=100).to(dev)
    eng = model.engine()
    staged = [eng.stage_captions(tok)] if eng.text_pack_enabled() else None

    def step():
        cap = tok
        if staged is not None:
            cap, staged[0] = staged[0], eng.stage_captions(tok)
        ts.forward(img, cap)
        ts.step(ts.backward())
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    # launch counts of one more step
    real, counts = hip.lib(), collections.Counter()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a, **k):
                counts[name] += 1
                return fn(*a, **k)
            return call
    hip._lib = Counting()
    step()
    torch.cuda.synchronize()
    hip._lib = real
    print(json.dumps({"arm": args.arm or ("p=%g" % args.drop_path), "bn": args.bn, "model": args.model, "batch": args.batch,
                      "drop_path": args.drop_path, "mode": args.mode if args.drop_path else None,
                      "step_ms_median": round(statistics.median(ms), 3), "step_ms_min": round(min(ms), 3), "step_ms_max": round(max(ms), 3),
                      "steps": args.steps, "library_calls_per_step": sum(counts.values()),
                      "gemm": counts["msclip_gemm"], "gemm_rowscale": counts["msclip_gemm_rowscale"],
                      "layernorm_bwd": counts["msclip_layernorm_bwd"], "layernorm_bwd_rowscale": counts["msclip_layernorm_bwd_rowscale"],
                      "cast_bf16": counts["msclip_cast_bf16"], "cast_bf16_colsum": counts["msclip_cast_bf16_colsum"],
                      "cast_bf16_colsum_rowscale": counts["msclip_cast_bf16_colsum_rowscale"], "colsum": counts["msclip_colsum"],
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
