"""A few optimizer steps of the MS-CLIP-S training step on synthetic image / caption pairs (random-init weights):

    python tools/train_synthetic.py --model b32-yfcc-msclips --batch 64 --steps 20 [--bn batch|frozen] [--lr 2e-5]
                                    [--accumulate K] [--clip-grad-norm X] [--ema-decay D] [--drop-path P [--drop-path-mode M]]
                                    [--optimizer adamw|lamb [--trust-clip]] [--nonfinite skip|raise]

--accumulate K: every optimizer step is ONE contrastive batch of K x --batch pairs, taken chunk by chunk through
TrainStep.accumulate (exact: every pair competes with all K x batch - 1 others); the loss printed is that batch's.

--clip-grad-norm X: TRAIN.CLIP_GRAD_NORM, the gradients are clipped to the global L2 norm X inside step() (on the device);
every fifth step also prints the norm before clipping.

--ema-decay D: TRAIN.EMA_DECAY, shadow weights follow the parameters inside step() (on the device); at the end the
inference-path loss is also printed under the shadow weights (TrainStep.ema_weights()), next to the live one.

--drop-path P: MODEL.SPEC.VISION.DROP_PATH, stochastic depth on both residual branches of every vision block (masks drawn on
the device, one draw per image -- or with --drop-path-mode position per token position, as the reference module does).  The
training losses then carry the masks' noise; the inference-path loss at the end does not.

--optimizer lamb: TRAIN.OPTIMIZER lamb, every parameter tensor's rate scaled by its trust ratio ||w|| / ||u|| inside step() (on
the device; --trust-clip caps the ratio at 1); every fifth step also prints the smallest and largest ratio of the tensors that
adapt.  LAMB's rates are larger than AdamW's: try --lr 2e-3.

--nonfinite skip|raise: TRAIN.SKIP_NONFINITE / TRAIN.DETECT_ANOMALY, a step whose gradient holds a NaN or an Inf leaves the model
and the optimizer state untouched (decided on the device; raise: step() then raises FloatingPointError naming the tensors); the
count of skipped steps is printed at the end.

Prints the contrastive loss of every step (the same fixed batches are cycled, so it has to fall), the step time and,
at the end, the inference-path loss of the first batch with the trained weights / running statistics.  One process per
GPU under torch.distributed.run for N > 1 (gradients are averaged over the ranks in 64 MiB buckets over RCCL)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()                           # HSA_KERNARG_POOL_SIZE: before the first HIP call of the process
import torch                                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b32-yfcc-msclips")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nbatches", type=int, default=2, help="distinct synthetic batches cycled through")
    ap.add_argument("--bn", choices=("batch", "frozen"), default="batch")
    ap.add_argument("--lr", type=float, default=2e-5)
    ap.add_argument("--steps-per-epoch", type=int, default=0,
                    help="> 0: follow the yaml's TRAIN.LR_SCHEDULER (timm cosine + warm-up, train.CosineSchedule) with this many steps per epoch")
    ap.add_argument("--accumulate", type=int, default=0,
                    help="K > 0: one optimizer step per K chunks of --batch pairs (TrainStep.accumulate; single process)")
    ap.add_argument("--clip-grad-norm", type=float, default=0.0,
                    help="X > 0: clip the gradients to the global L2 norm X inside step() (TRAIN.CLIP_GRAD_NORM; 0 = off)")
    ap.add_argument("--ema-decay", type=float, default=0.0,
                    help="D in (0, 1): keep an exponential moving average of the weights inside step() (TRAIN.EMA_DECAY; 0 = off)")
    ap.add_argument("--drop-path", type=float, default=0.0,
                    help="P in (0, 1): stochastic depth on the vision blocks' residual branches (MODEL.SPEC.VISION.DROP_PATH; 0 = off)")
    ap.add_argument("--drop-path-mode", choices=("sample", "position"), default="sample",
                    help="one draw per image (sample) or per token position, shared by the batch (position: the reference module's layout)")
    ap.add_argument("--optimizer", choices=("adamw", "lamb"), default="adamw", help="TRAIN.OPTIMIZER (lamb: per-tensor trust ratios)")
    ap.add_argument("--trust-clip", action="store_true", help="lamb: cap the trust ratio at 1 (OPTIMIZER_ARGS.trust_clip)")
    ap.add_argument("--nonfinite", choices=("skip", "raise"), default=None,
                    help="skip the optimizer step on NaN / Inf gradients (TRAIN.SKIP_NONFINITE), or skip and raise (TRAIN.DETECT_ANOMALY)")
    args = ap.parse_args()
    from msclip_amd import comm as C, synth, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    C.init_distributed("nccl")
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if dist.is_initialized():                              # a process group exists: leave the legacy default stream (once, explicitly)
        from msclip_amd import hip
        hip.use_compute_stream(dev)
    cfg = named_config(args.model, ["TRAIN.CLIP_GRAD_NORM", str(args.clip_grad_norm), "TRAIN.EMA_DECAY", str(args.ema_decay),
                                    "MODEL.SPEC.VISION.DROP_PATH", str(args.drop_path)]
                       + (["TRAIN.OPTIMIZER", "lamb", "TRAIN.OPTIMIZER_ARGS.trust_clip", str(args.trust_clip)] if args.optimizer == "lamb" else [])
                       + ({"skip": ["TRAIN.SKIP_NONFINITE", "True"], "raise": ["TRAIN.DETECT_ANOMALY", "True"]}.get(args.nonfinite, [])))
    from bench import load_schema
    model = get_clip_model(cfg)
    model.load_state_dict(synth.synth_state_dict(load_schema(args.model), seed=0), strict=True)
    model = model.to(dev).eval()
    ts = train.from_config(model, cfg, bn=args.bn, drop_path_mode=args.drop_path_mode)
    ts.lr = ts.lr_share = args.lr                          # (the schedule scales these base rates epoch by epoch)
    rank = C.comm.rank
    data = [(synth.synth_images(args.batch, seed=1000 * rank + 10 + i).to(dev),
             synth.synth_tokens(args.batch, seed=1000 * rank + 100 + i).to(dev)) for i in range(args.nbatches)]
    K = args.accumulate
    if K > 0:                                              # nbatches big batches of K chunks each
        data = [[(synth.synth_images(args.batch, seed=10 + K * i + k).to(dev), synth.synth_tokens(args.batch, seed=100 + K * i + k).to(dev))
                 for k in range(K)] for i in range(args.nbatches)]
    losses = []
    for step in range(args.steps):
        if K == 0:
            img, tok = data[step % args.nbatches]
        if args.steps_per_epoch > 0 and step % args.steps_per_epoch == 0:
            ts.set_epoch(step // args.steps_per_epoch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if K > 0:
            loss, grads = ts.accumulate(data[step % args.nbatches])
            ts.step(grads)
        else:
            loss = ts.forward(img, tok)
            ts.step(ts.backward())
        torch.cuda.synchronize()
        losses.append(float(loss))
        ms = 1e3 * (time.perf_counter() - t0)
        note = ""
        if ts.last_grad_norm is not None and step % 5 == 0:   # one more read on a step that has just read the loss
            note = f"  grad norm {ts.last_grad_norm.item():.4g}" + (f" (clipped to {ts.clip_grad_norm:g})" if ts.clip_grad_norm else "")
        if ts.last_trust_ratio is not None and step % 5 == 0:
            adapting = torch.stack([ts.last_trust_ratio[k] for k, _, _, wd in ts.param_groups() if wd != 0.0 or ts.always_adapt])
            note += f"  trust ratio {adapting.min().item():.3g} .. {adapting.max().item():.3g}"
        if rank == 0:
            print(f"step {step:3d}  loss {losses[-1]:.4f}  {ms:7.1f} ms{note}", flush=True)
    # the inference-path loss gathers features and all-reduces its partial sums (GATHER_TENSORS: True): EVERY rank runs it,
    # rank 0 prints it
    first = data[0][0] if K > 0 else data[0]
    inf = float(model.contrastive_loss(*first))
    ema_inf = None
    if ts.ema_shadow is not None:
        with ts.ema_weights():
            ema_inf = float(model.contrastive_loss(*first))
    ok = all(l == l for l in losses) and min(losses[-args.nbatches:]) < losses[0]
    if rank == 0:
        print(f"first {'chunk' if K > 0 else 'batch'} through the inference path (running statistics): loss {inf:.4f}"
              + (f", under the EMA weights (decay {ts.ema_decay:g}, {ts.ema_updates} updates) {ema_inf:.4f}" if ema_inf is not None else ""))
        if ts.nonfinite is not None:
            print(f"non-finite guard ({ts.nonfinite}): {ts.skipped_steps} of {ts.steps} steps skipped")
        print("OK" if ok else "FAILED: the loss did not fall")
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
