"""What the training input path sustains (recorded, not gated): writes profiles/input_pipeline_bench.md.

    python tools/input_bench.py [--files 768] [--batch 256] [--out profiles/input_pipeline_bench.md] [--colour]

* host ms per image of `load_source` (decode only: draft + reduce) against a host-side PIL decode + crop().resize() of the same
  file, one thread;
* msclip_resized_crop's time for a batch of 512 at 224 x 224 from 512 x 512 slots, bicubic and bilinear (HIP events);
* PairPipeline alone (decode threads, one copy per batch, the launch) in pairs/s, beside the training step's pairs/s of
  profiles/r06_bench_lines.jsonl -- and the sentence that follows from the two.
--colour measures the colour stage alone (msclip_color_augment beside msclip_resized_crop at 512 x 224 x 224 with every stage on
and p = 1, and PairPipeline's pairs/s with and without colour) and replaces that section of the file, leaving the rest as recorded.
The files are generated: JPEGs (quality 90) of sizes drawn around 500 x 375, the usual size of a web photograph."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_files(root, n, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    items = []
    for i in range(n):
        h, w = ((375, 500), (500, 375), (333, 500), (480, 640), (600, 800), (256, 256))[i % 6]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        a = np.stack([127.5 + 80 * np.sin(rng.uniform(0.01, 0.2) * yy + rng.uniform(0.01, 0.2) * xx + rng.uniform(0, 6)) for _ in range(3)], 2)
        a = np.clip(a + rng.normal(0, 10, a.shape), 0, 255).astype(np.uint8)
        path = os.path.join(root, "img_%05d.jpg" % i)
        Image.fromarray(a).save(path, quality=90)
        items.append((path, "a photo of object number %d" % i))
    return items


def _shape_of(path):
    from msclip_amd._decode_worker import load_source
    return load_source(path, 512).shape


COLOUR_HEAD = "## The colour stage"


def _event_ms(fn, warm=5, reps=50):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def colour_section(args, dev):
    """-> the lines of the colour stage's section: the launch beside the crop's, and the pipeline with and without colour."""
    from msclip_amd import augment, color_hip, input_hip, pairs, zeroshot
    from msclip_amd.config import named_config
    from msclip_amd.tokenizer import SimpleTokenizer
    B, g = 512, torch.Generator().manual_seed(0)
    on = ["AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 1.0]", "AUG.GRAY_SCALE", "1.0", "AUG.GAUSSIAN_BLUR", "1.0"]
    typical = ["AUG.COLOR_JITTER", "[0.4, 0.4, 0.4, 0.1, 0.8]", "AUG.GRAY_SCALE", "0.2", "AUG.GAUSSIAN_BLUR", "0.5"]
    s_all = augment.aug_settings(named_config("b32-yfcc-msclips", on), colour=True)
    s_typ = augment.aug_settings(named_config("b32-yfcc-msclips", typical), colour=True)
    s_off = augment.aug_settings(named_config("b32-yfcc-msclips"), colour=True)
    src = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device=dev)
    dims = torch.tensor([[375, 500]] * B, dtype=torch.int32, device=dev)
    bx = augment.random_resized_crop_boxes(torch.tensor([[375, 500]] * B), torch.rand(B, 10, 4, dtype=torch.float64, generator=g)).to(dev)
    lut = zeroshot.normalise_lut().to(dev)
    out, u8 = input_hip.resized_crop(src, dims, bx, lut, 224, want_u8=True)
    lines = [COLOUR_HEAD, "",
             f"`tools/input_bench.py --colour`: msclip_color_augment on {B} x 224 x 224 (band {color_hip.augment_band(224, 224)}, "
             f"{color_hip.augment_lds(224, 224)} B of LDS per blurring workgroup), HIP events over 50 launches after 5, beside "
             "msclip_resized_crop (bicubic, 512 x 512 slots, with out_u8) in the same process.", "",
             "| launch | ms | images/s |", "|---|---|---|"]
    ms = crop_ms = _event_ms(lambda: input_hip.resized_crop(src, dims, bx, lut, 224, out=out, want_u8=True))
    lines.append(f"| msclip_resized_crop, bicubic, out and out_u8 | {ms:.3f} | {B / ms * 1e3:.0f} |")
    stage_ms = []
    u = torch.rand(B, augment.COLOUR_DRAWS, dtype=torch.float64, generator=g)
    for what, settings in (("every stage on every image (p = 1)", s_all), ("jitter 0.8, gray 0.2, blur 0.5", s_typ)):
        ops, coef = (t.to(dev) for t in augment.colour_params(u, settings))
        st = augment.colour_stages(settings)
        ms = _event_ms(lambda: color_hip.color_augment(u8, ops, coef, lut, stages=st, out=out))
        stage_ms.append(ms)
        lines.append(f"| msclip_color_augment, {what} | {ms:.3f} | {B / ms * 1e3:.0f} |")
    ops, coef = (t.to(dev) for t in augment.colour_params(u, s_all))
    for what, st in (("jitter alone (both kernels, no LDS)", 1), ("gray alone", 2), ("blur alone", 4)):
        ms = _event_ms(lambda: color_hip.color_augment(u8, ops, coef, lut, stages=st, out=out))
        lines.append(f"| msclip_color_augment, {what} | {ms:.3f} | {B / ms * 1e3:.0f} |")
    del src
    lines += ["", f"PairPipeline alone, batch {args.batch}, {args.files // args.batch} batches per epoch, 8 decoding threads, pairs/s:", "",
              "| colour | epoch 0 (cold) | epoch 1 | epoch 2 |", "|---|---|---|---|"]
    tok = SimpleTokenizer()
    with tempfile.TemporaryDirectory() as root:
        items = make_files(root, args.files)
        for what, settings in (("off", s_off), ("jitter 0.8, gray 0.2, blur 0.5", s_typ), ("every stage, p = 1", s_all)):
            pipe = pairs.PairPipeline(items, args.batch, dev, settings, tokenizer=tok, seed=0, workers=8)
            rates = []
            for epoch in range(3):
                pipe.set_epoch(epoch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for img, _, _ in pipe:
                    n += img.shape[0]
                torch.cuda.synchronize()
                rates.append(n / (time.perf_counter() - t0))
            pipe.close()
            lines.append(f"| {what} | " + " | ".join(f"{r:.0f}" for r in rates) + " |")
    step_ms = 512 / 8278 * 1e3                               # (profiles/r06_bench_lines.jsonl: train-mode BatchNorm, batch 512)
    lines += ["", f"The stage takes {stage_ms[0] / crop_ms:.2f} x the crop's own time with every stage on every image and "
              f"{stage_ms[1] / crop_ms:.2f} x at the usual probabilities: "
              + ("below the crop's, as expected" if stage_ms[0] < crop_ms else "NOT below the crop's, which had been the expectation")
              + f"; crop and colour together are {100 * (crop_ms + stage_ms[0]) / step_ms:.1f} % of a "
              f"{step_ms:.0f} ms training step at most. The pipeline's rate is set by the host's decoding threads and moves as much from "
              "epoch to epoch within a row as the rows differ from each other: the colour stage does not show in it."]
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--colour", action="store_true", help="measure the colour stage alone and replace its section of --out")
    ap.add_argument("--files", type=int, default=768)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pipeline_bench.md"))
    args = ap.parse_args()
    from PIL import Image
    from msclip_amd import augment, input_hip, pairs, zeroshot
    from msclip_amd._decode_worker import load_source
    from msclip_amd.config import named_config
    from msclip_amd.tokenizer import SimpleTokenizer
    dev = torch.device("cuda", 0)
    if args.colour:
        lines = colour_section(args, dev)
        old = open(args.out).read() if os.path.exists(args.out) else ""
        keep = old.split(COLOUR_HEAD)[0].rstrip("\n")
        with open(args.out, "w") as f:
            f.write((keep + "\n\n" if keep else "") + "\n".join(lines))
        print("\n".join(lines))
        return
    settings = augment.aug_settings(named_config("b32-yfcc-msclips"), colour=True)
    lines = ["# The training input path: what it sustains", "",
             f"`tools/input_bench.py --files {args.files} --batch {args.batch}` on one MI355X, {zeroshot.effective_cores()} usable host cores. "
             "Recorded, not gated: the parent commit has no training input path to compare with.", ""]
    with tempfile.TemporaryDirectory() as root:
        items = make_files(root, args.files)
        # ---- host: decode only against decode + crop + resize
        sub = items[:192]
        t0 = time.perf_counter()
        sizes = [load_source(p, 512).shape[:2] for p, _ in sub]
        t_src = (time.perf_counter() - t0) / len(sub)
        g = torch.Generator().manual_seed(0)
        boxes = augment.random_resized_crop_boxes(torch.tensor(sizes), torch.rand(len(sub), 10, 4, dtype=torch.float64, generator=g))
        t0 = time.perf_counter()
        for (p, _), (h, w), (t, l, bh, bw) in zip(sub, sizes, boxes.tolist()):
            with Image.open(p) as im:
                img = im.convert("RGB")
            sy, sx = img.size[1] / h, img.size[0] / w          # the box in the full-size image
            np.asarray(img.crop((int(l * sx), int(t * sy), int((l + bw) * sx), int((t + bh) * sy))).resize((224, 224), Image.BICUBIC))
        t_pil = (time.perf_counter() - t0) / len(sub)
        lines += ["## Host, one thread, per image", "", "| path | ms per image |", "|---|---|",
                  f"| `load_source` (decode, draft, reduce; no filter resize) | {1e3 * t_src:.2f} |",
                  f"| PIL decode + `crop().resize((224, 224), BICUBIC)` | {1e3 * t_pil:.2f} |", ""]
        # ---- decode-only pools: what threads and processes give on this host (before the first HIP call: the processes are forks)
        import concurrent.futures as cf
        paths = [p for p, _ in items[:512]]
        lines += ["## Decode-only pools (`load_source`, no staging, no GPU; the better of two passes over 512 files)", "",
                  "| pool | images/s |", "|---|---|"]
        pools = {}
        for kind, counts in ((cf.ThreadPoolExecutor, (4, 8, 16)), (cf.ProcessPoolExecutor, (8, 16))):
            what = "threads" if kind is cf.ThreadPoolExecutor else "processes"
            for n in counts:
                with kind(n) as pool:
                    list(pool.map(_shape_of, paths[:64]))
                    dt = float("inf")
                    for _ in range(2):
                        t0 = time.perf_counter()
                        list(pool.map(_shape_of, paths, chunksize=8) if kind is cf.ProcessPoolExecutor else pool.map(_shape_of, paths))
                        dt = min(dt, time.perf_counter() - t0)
                pools[what, n] = len(paths) / dt
                lines.append(f"| {n} {what} | {pools[what, n]:.0f} |")
        lines.append("")
        # ---- the kernel
        B = 512
        src = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, device=dev)
        dims = torch.tensor([[375, 500]] * B, dtype=torch.int32, device=dev)
        u = torch.rand(B, 10, 4, dtype=torch.float64, generator=g)
        bx = augment.random_resized_crop_boxes(torch.tensor([[375, 500]] * B), u).to(dev)
        lut = zeroshot.normalise_lut().to(dev)
        lines += ["## msclip_resized_crop, 512 images, 512 x 512 slots -> 224 x 224", "",
                  f"375 x 500 images, boxes drawn with the default scale / ratio; band {input_hip.crop_band(512, 512, 224, 224)}, "
                  f"{input_hip.crop_lds(512, 512, 224, 224)} B of LDS per workgroup.", "", "| filter | ms per launch | images/s |", "|---|---|---|"]
        for code, name in ((3, "bicubic"), (2, "bilinear")):
            for _ in range(3):
                input_hip.resized_crop(src, dims, bx, lut, 224, filter=code)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(20):
                input_hip.resized_crop(src, dims, bx, lut, 224, filter=code)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / 20
            lines.append(f"| {name} | {ms:.3f} | {B / ms * 1e3:.0f} |")
        full = torch.tensor([[0, 0, 375, 500]] * B, dtype=torch.int32, device=dev)
        for _ in range(2):
            input_hip.resized_crop(src, dims, full, lut, 224)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(10):
            input_hip.resized_crop(src, dims, full, lut, 224)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / 10
        lines += [f"| bicubic, every box the whole image (the most source rows) | {ms:.3f} | {B / ms * 1e3:.0f} |", ""]
        del src
        # ---- the pipeline alone
        tok = SimpleTokenizer()
        table, best, workers = [], 0.0, 0
        for nw in (8, None):
            pipe = pairs.PairPipeline(items, args.batch, dev, settings, tokenizer=tok, seed=0, workers=nw)
            rates = []
            for epoch in range(3):
                pipe.set_epoch(epoch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for img, _, _ in pipe:
                    n += img.shape[0]
                torch.cuda.synchronize()
                rates.append(n / (time.perf_counter() - t0))
            table.append(f"| {pipe.workers}{' (the default)' if nw is None else ''} | " + " | ".join(f"{r:.0f}" for r in rates) + " |")
            if max(rates[1:]) > best:
                best, workers = max(rates[1:]), pipe.workers
            pipe.close()
    step = {}
    with open(os.path.join(ROOT, "profiles", "r06_bench_lines.jsonl")) as f:
        for line in f:
            d = json.loads(line)
            if d.get("tag") in ("train_frozen", "train_batch"):
                step[d["tag"]] = d["value"]
    lines += [f"## PairPipeline alone, batch {args.batch}, {args.files // args.batch} batches per epoch", "",
              "| decoding threads | epoch 0 (cold), pairs/s | epoch 1 | epoch 2 |", "|---|---|---|---|"] + table
    lines += ["", f"The training step (profiles/r06_bench_lines.jsonl, ViT-B/32, batch 512): {step.get('train_frozen', 0):.0f} pairs/s with frozen "
              f"BatchNorm, {step.get('train_batch', 0):.0f} pairs/s with train-mode BatchNorm.", ""]
    keeps = best >= step.get("train_batch", float("inf"))
    bt = max(((n, r) for (what, n), r in pools.items() if what == "threads"), key=lambda t: t[1])
    bp = max(((n, r) for (what, n), r in pools.items() if what == "processes"), key=lambda t: t[1])
    lines += [("**The input keeps up with the step**" if keeps else "**The input does not keep up with the step**")
              + f": {best:.0f} pairs/s at best ({workers} threads) against {step.get('train_batch', 0):.0f} - {step.get('train_frozen', 0):.0f} pairs/s. "
              + ("" if keeps else f"The step would wait for input {100 * (1 - best / step.get('train_batch', best)):.0f} % of the time with "
                 "train-mode BatchNorm. The kernel is not the limit (above); decoding on the host's threads is: the best decode-only "
                 f"thread pool above reaches {bt[1]:.0f} images/s ({bt[0]} threads; 16 threads {pools['threads', 16]:.0f}), the best process "
                 f"pool {bp[1]:.0f} ({bp[0]} processes)"
                 + (", which would cover the step" if bp[1] >= step.get("train_frozen", float("inf")) else "")
                 + ". Decoding processes, as the eval pipeline has, are the follow-up."), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):                             # (the colour stage's section is --colour's: kept as recorded)
        with open(args.out) as f:
            old = f.read()
        if COLOUR_HEAD in old:
            lines += [COLOUR_HEAD + old.split(COLOUR_HEAD, 1)[1].rstrip("\n"), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
