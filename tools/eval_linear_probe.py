"""Linear-probe evaluation CLI: the second number the reference's README reports for every checkpoint ("LP"), measured the way
CLIP's protocol states it -- a softmax classifier on the frozen, un-normalised projected image features, L-BFGS, max_iter 1000,
scikit-learn C = 0.316 (or a sweep), no augmentation.  The reference ships no linear-probe code: the protocol is unpinned.

    python tools/eval_linear_probe.py --model experiments/model/b32-yfcc-msclips.yaml --train-root <dir> --val-root <dir>
                                      [--csk 0.316 | --sweep] [--metric mean_per_class] [--max-images N] [--random-init]
                                      [--cache DIR] [KEY VALUE ...]

Both roots are ImageFolder trees with the same class directories.  --sweep chooses l2 on a held-out fifth of the training rows
from a log-spaced grid (--sweep-points values of Csk between 1e-6 and 1e6, as CLIP's appendix describes) and refits on all of
them.  --cache DIR keeps the extracted features (train.npz, val.npz), keyed by the checkpoint's weights and the file lists.  The
config is built like tools/eval_zeroshot.py's (model yaml over the defaults, trailing KEY VALUE overrides); the checkpoint comes
from --ckpt or MODEL.PRETRAINED_MODEL.  Prints one JSON line with the result.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msclip_amd import checkpoint, linear_probe                  # noqa: E402
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model      # noqa: E402
from msclip_amd.config import default_config, update_config      # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Linear-probe Eval")
    ap.add_argument("--model", required=True, type=str, help="Evaluation model configure file name")
    ap.add_argument("--train-root", required=True, help="ImageFolder tree the classifier is fitted on")
    ap.add_argument("--val-root", required=True, help="ImageFolder tree it is scored on (same class directories)")
    ap.add_argument("--csk", type=float, default=0.316, help="scikit-learn's C; l2 = 1 / (C * N)")
    ap.add_argument("--sweep", action="store_true", help="choose l2 on a held-out fifth of the training rows instead of --csk")
    ap.add_argument("--sweep-points", type=int, default=13, help="grid points of --sweep, log-spaced Csk in [1e-6, 1e6]")
    ap.add_argument("--metric", default="accuracy", choices=linear_probe.METRICS)
    ap.add_argument("--normalize", action="store_true", help="unit-norm features (default: the raw projection, CLIP's protocol)")
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--ckpt", default=None, help="defaults to MODEL.PRETRAINED_MODEL of the yaml")
    ap.add_argument("--random-init", action="store_true", help="no checkpoint: plumbing run on random-init weights")
    ap.add_argument("--max-images", type=int, default=None, help="a strided subset of each tree")
    ap.add_argument("--cache", default=None, help="directory for the extracted features")
    ap.add_argument("--workers", type=int, default=None, help="decoding threads of the input pipeline")
    ap.add_argument("--processes", type=int, default=None, help="decoding PROCESSES instead of threads")
    ap.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)
    return ap.parse_args(argv)


def build_config(model_yaml, opts):
    class _A:
        pass
    a = _A()
    config = default_config()
    a.cfg, a.opts = model_yaml, opts
    update_config(config, a)
    config.defrost()
    config.NAME = ""
    config.freeze()
    return config


def l2_grid(points, n):
    """Csk log-spaced over [1e-6, 1e6] -> l2 = 1 / (Csk n), descending."""
    import numpy as np
    return [linear_probe.l2_from_csk(c, n) for c in np.logspace(-6, 6, int(points))]


def run(argv=None, log=print):
    args = parse_args(argv)
    config = build_config(args.model, args.opts or [])
    model = get_clip_model(config)
    if args.random_init:
        log("=> WARNING: --random-init, evaluating untrained weights (plumbing run)")
    else:
        model_file = args.ckpt or config.MODEL.PRETRAINED_MODEL
        log("=> load model file: {}".format(model_file))
        checkpoint.load_pretrained(model, model_file)
    model = model.cuda().eval()
    grid = None
    if args.sweep:
        from msclip_amd import zeroshot
        n = len(zeroshot.image_folder(args.train_root)[1])
        n = min(n, args.max_images) if args.max_images else n
        grid = l2_grid(args.sweep_points, n - n // 5)
    res = linear_probe.evaluate(model, args.train_root, args.val_root, csk=args.csk, l2_grid=grid, metric=args.metric,
                                batch_size=config.TEST.BATCH_SIZE_PER_GPU, normalize=args.normalize, workers=args.workers,
                                processes=args.processes, max_images=args.max_images, cache=args.cache, max_iter=args.max_iter,
                                chunk_rows=args.chunk_rows, size=config.TEST.IMAGE_SIZE[0], mean=config.INPUT.MEAN,
                                std=config.INPUT.STD, log=log)
    res.pop("P")
    if res.get("per_l2"):
        res["per_l2"] = [{k: v for k, v in p.items() if k != "P"} for p in res["per_l2"]]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    run()
