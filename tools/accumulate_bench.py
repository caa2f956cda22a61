"""Time and memory of TrainStep.accumulate on one MI355X:

    python tools/accumulate_bench.py --model b32-yfcc-msclips --batch 512 --chunks 8 [--bn batch] [--precision bf16]

Prints one JSON line: milliseconds per optimizer step and per chunk of accumulate() + step() over K chunks of --batch pairs,
the share of the feature pass, the head, the gradient pass and the msclip_grad_accumulate launches (device events at the
phase boundaries, TrainStep.phase_events), the one-shot step (forward + backward + step) of one chunk for comparison,
max_memory_allocated of both, and the accumulate kernel against a loop of ATen adds over the same tensors."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import torch                                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=512, help="pairs per chunk")
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--bn", choices=("batch", "frozen"), default="batch")
    ap.add_argument("--precision", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--memory-chunks", type=int, nargs="*", default=[2, 8], help="K values whose peak memory is recorded")
    args = ap.parse_args()
    from bench import load_schema
    from msclip_amd import hip, synth, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = get_clip_model(named_config(args.model, ["MODEL.SPEC.PRECISION", args.precision] if args.precision else None))
    model.load_state_dict(synth.synth_state_dict(load_schema(args.model), seed=0), strict=True)
    model = model.to(dev).eval()
    ts = train.from_config(model, named_config(args.model), bn=args.bn)
    B, K = args.batch, args.chunks
    kmax = max([K] + args.memory_chunks)
    chunks = [(synth.synth_images(B, seed=10 + k).to(dev), synth.synth_tokens(B, seed=100 + k).to(dev)) for k in range(kmax)]
    rec = dict(model=args.model, bn=args.bn, chunk=B, chunks=K, params=sum(p.numel() for p in model.parameters()))

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    def one_shot():
        ts.forward(*chunks[0])
        ts.step(ts.backward())

    def accumulated(k=K):
        loss, grads = ts.accumulate(chunks[:k])
        ts.step(grads)

    # ---- peak memory first (fresh allocator statistics per measurement)
    def peak(fn):
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev)
    rec["peak_bytes_one_shot"] = peak(one_shot)
    rec["peak_bytes_accumulate"] = {str(k): peak(lambda k=k: accumulated(k)) for k in args.memory_chunks}
    E = ts.eng.E
    rec["bank_bytes_per_modality"] = {str(k): k * B * 2 * E * 2 for k in args.memory_chunks}
    rec["head_block_bytes"] = {str(k): B * k * B * 4 for k in args.memory_chunks}
    rec["accumulator_bytes"] = ts._acc.arena.numel() * 4
    # ---- time, alternating
    a, b = [], []
    for _ in range(2):
        a.append(timed(one_shot, args.steps * 2, args.warmup))
        b.append(timed(accumulated, args.steps, args.warmup))
    rec["one_shot_ms"] = a
    rec["accumulate_step_ms"] = b
    rec["accumulate_ms_per_chunk"] = [x / K for x in b]
    rec["ratio_per_pair"] = min(b) / K / min(a)
    # ---- phases by device events
    ts.phase_events = []
    accumulated()
    torch.cuda.synchronize()
    ev, ts.phase_events = ts.phase_events, None
    span = lambda i: ev[i - 1][1].elapsed_time(ev[i][1])
    names = [n for n, _ in ev]
    acc_ms = [span(i) for i, n in enumerate(names) if n == "accumulate"]
    total = ev[0][1].elapsed_time(ev[-1][1])
    rec["phase_ms"] = dict(features=span(names.index("features")), head=span(names.index("head")),
                           gradient_pass=ev[names.index("head")][1].elapsed_time(ev[-1][1]) - sum(acc_ms),
                           accumulate_launches=sum(acc_ms), total=total)
    # ---- the kernel: launches per chunk, microseconds, bytes / time; against a loop of ATen adds
    acc = ts._acc
    sizes = [acc.views[k].numel() for k in acc.keys]
    launches, nt, nb = 0, 0, 0
    for n in sizes:                                        # the table-filling rule of msclip_grad_accumulate (36 tensors, 768 pieces of 32 K)
        c, chunks_ = 0, (n + 32767) // 32768
        while c < chunks_:
            if nt == 36 or nb == 768:
                launches, nt, nb = launches + 1, 0, 0
            take = min(chunks_ - c, 768 - nb)
            c, nb, nt = c + take, nb + take, nt + 1
    launches += 1 if nb else 0
    gs = [torch.randn(n, device=dev) for n in sizes]
    flat = [acc.views[k].view(-1) for k in acc.keys]

    def dev_ms(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        s, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e_.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e_) / reps
    k1 = dev_ms(lambda: acc.plan.run(gs, 1))
    k0 = dev_ms(lambda: acc.plan.run(gs, 0))

    def aten():
        for t, g in zip(flat, gs):
            t.add_(g)
    at = dev_ms(aten, reps=2)
    nel = sum(sizes)
    rec["kernel"] = dict(tensors=len(sizes), elements=nel, launches_per_chunk=launches, mode1_us=1e3 * k1, mode0_us=1e3 * k0,
                         mode1_TBps=12 * nel / (k1 * 1e-3) / 1e12, mode0_TBps=8 * nel / (k0 * 1e-3) / 1e12,
                         aten_loop_us=1e3 * at, aten_loop_TBps=12 * nel / (at * 1e-3) / 1e12)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
