"""Train MS-CLIP-S on image files: a TSV of `relative/path<TAB>caption` lines through msclip_amd.pairs.PairPipeline (decode on the
host; random-resized crop, flip and normalisation in one launch on the device, colour jitter / grayscale / Gaussian blur in a second
stage where the config turns one on) into the training step.

    python tools/train_pairs.py --model <yaml or name> --pairs <tsv> --root <dir> --epochs N --batch B
                                [--bn batch|frozen] [--resume ckpt] [--save ckpt] [--random-init] [--steps K] [--seed S]
                                [--workers W] [--slot 512] [KEY VALUE ...]

The yaml's optimizer block, schedule, EMA, clipping, stochastic depth and guard are train.from_config's; the augmentation is
augment.aug_settings' (AUG.SCALE, AUG.RATIO, TRAIN.IMAGE_SIZE, INPUT.MEAN / STD, AUG.INTERPOLATION, AUG.FLIP_PROB, AUG.COLOR_JITTER,
AUG.GRAY_SCALE, AUG.GAUSSIAN_BLUR; any other augmentation switch that is on is refused by name).  KEY VALUE pairs override the yaml (e.g. PRINT_FREQ 1 AUG.FLIP_PROB 0.5).

--save ckpt writes the reference's resumable checkpoint (train.save_checkpoint) when the run ends and the input pipeline's state
(epoch, position, seed, generator) beside it as <ckpt>.input.pt; --resume ckpt loads both and continues with the batches the
uninterrupted run would have seen.  --steps K ends the run after K optimizer steps.  --random-init: no pretrained weights.
Prints the loss and pairs/s every PRINT_FREQ steps (default 20).  One process per GPU under torch.distributed.run for N > 1."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()                           # HSA_KERNARG_POOL_SIZE: before the first HIP call of the process
import torch                                             # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, help="a model yaml, or the name of one under experiments/model")
    ap.add_argument("--pairs", required=True, help="TSV: relative/path<TAB>caption")
    ap.add_argument("--root", default="", help="directory the TSV's paths are relative to")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256, help="pairs per step and GPU")
    ap.add_argument("--bn", choices=("batch", "frozen"), default="batch")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--steps", type=int, default=0, help="K > 0: stop after K optimizer steps of this run")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=None, help="decoding threads (default: one per usable core, at most 16)")
    ap.add_argument("--slot", type=int, default=512, help="largest side a decoded image keeps")
    ap.add_argument("--bpe", default=None, help="merges table (default: the packaged one)")
    ap.add_argument("opts", help="KEY VALUE pairs that override the yaml", default=None, nargs=argparse.REMAINDER)
    args = ap.parse_args(argv)
    from msclip_amd import augment, checkpoint, comm as C, config as cfgmod, pairs, train
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.tokenizer import SimpleTokenizer
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    C.init_distributed("nccl")
    dev = torch.device("cuda", local)
    if torch.distributed.is_initialized():                 # a process group exists: leave the legacy default stream
        from msclip_amd import hip
        hip.use_compute_stream(dev)
    rank, world = C.comm.rank, C.comm.world_size
    log = print if rank == 0 else (lambda *a, **k: None)
    cfg = cfgmod.load_config(args.model, args.opts) if os.path.exists(args.model) else cfgmod.named_config(args.model, args.opts)
    settings = augment.aug_settings(cfg, colour=True)      # (refuses what is not implemented before anything is built)
    torch.manual_seed(args.seed)
    model = get_clip_model(cfg)
    if args.random_init:
        log("=> WARNING: --random-init, training from untrained weights")
    elif not args.resume:
        log("=> load model file: {}".format(cfg.MODEL.PRETRAINED_MODEL))
        checkpoint.load_pretrained(model, cfg.MODEL.PRETRAINED_MODEL)
    model = model.to(dev).eval()
    ts = train.from_config(model, cfg, bn=args.bn)
    items = pairs.read_pairs(args.pairs, args.root)
    pipe = pairs.PairPipeline(items, args.batch, dev, settings, tokenizer=SimpleTokenizer(args.bpe), seed=args.seed,
                              workers=args.workers, slot=args.slot, rank=rank, world=world)
    log(f"=> {len(items)} pairs, {len(pipe)} steps per epoch at {args.batch} pairs x {world} GPU(s); crop scale {settings['scale']}, "
        f"ratio ({settings['ratio'][0]:.3f}, {settings['ratio'][1]:.3f}), size {settings['size']}, filter {settings['interpolation']}, "
        f"flip {settings['flip_prob']:g}; colour jitter {list(settings['color_jitter'])}, gray {settings['gray_scale']:g}, "
        f"blur {settings['gaussian_blur']:g}; {pipe.workers} decoding threads")
    if len(pipe) == 0:
        raise SystemExit(f"{args.pairs}: fewer pairs than one batch of {args.batch} x {world}")
    step = 0
    if args.resume:
        step = train.resume_checkpoint(model, ts, args.resume)
        pipe.load_state_dict(torch.load(args.resume + ".input.pt", map_location="cpu", weights_only=False))
        log(f"=> resumed {args.resume}: step {step}, epoch {pipe.epoch}, batch {pipe.pos} of {len(pipe)}")
    freq = max(1, int(cfg.get("PRINT_FREQ", 20)))
    done, pending, ok = 0, [], True
    t0, n0 = time.perf_counter(), 0
    resumed_epoch = pipe.epoch if args.resume else None
    for epoch in range(pipe.epoch, args.epochs):
        if epoch != resumed_epoch:
            pipe.set_epoch(epoch)
        ts.set_epoch(epoch)
        for img, tok, index in pipe:
            if done == 0:
                log("first batch indices: " + " ".join(str(int(i)) for i in index))
            loss = ts.forward(img, tok)
            ts.step(ts.backward())
            pending.append((step, loss))
            step += 1
            done += 1
            if done % freq == 0 or (args.steps and done >= args.steps):
                torch.cuda.synchronize(dev)
                dt, t0 = time.perf_counter() - t0, time.perf_counter()
                for s, l in pending:
                    ok = ok and bool(torch.isfinite(l).all())
                    log(f"epoch {epoch} step {s:6d}  loss {float(l):.4f}")
                log(f"    {(done - n0) * args.batch * world / max(dt, 1e-9):.0f} pairs/s over the last {done - n0} steps")
                pending, n0 = [], done
            if args.steps and done >= args.steps:
                break
        if args.steps and done >= args.steps:
            break
    torch.cuda.synchronize(dev)
    for s, l in pending:
        ok = ok and bool(torch.isfinite(l).all())
        log(f"step {s:6d}  loss {float(l):.4f}")
    if args.save:
        train.save_checkpoint(model, ts, args.save, step - 1, model_name=cfg.MODEL.NAME)
        if rank == 0:
            torch.save(pipe.state_dict(), args.save + ".input.pt")
        log(f"=> saved {args.save} and {args.save}.input.pt (step {step}, epoch {pipe.epoch}, batch {pipe.pos})")
    pipe.close()
    log("OK" if ok else "FAILED: a loss was not finite")
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
