"""Image / caption pairs from files into the training step: decode on the host, everything else on the device.

    read_pairs(manifest, root)  ->  [(path, caption)]        a UTF-8 TSV, `relative/path<TAB>caption` per line
    PairPipeline(items, batch_size, device, settings)        iterate: (img [B, 3, S, S] fp32, tok int64 [B, 77], index)

The host's cores are the scarce resource, so the worker threads only DECODE (`_decode_worker.load_source`: JPEG draft mode, an
integer `reduce`, no filter resize), and one task per batch tokenizes its captions.  A decoded image lands in its slot of a pinned staging buffer; the buffer's
header holds the batch's token ids, image sizes, crop boxes and flip flags, so that a batch is ONE host-to-device copy on a copy
stream.  The random-resized crop, the flip and the normalisation are one launch on the device (input_hip.resized_crop).  The boxes
are computed on the host (augment.random_resized_crop_boxes) from uniforms of a CPU generator the pipeline owns, once the workers
have reported the sizes: nothing is read back from the device.  Where the settings turn a colour stage on (AUG.COLOR_JITTER,
AUG.GRAY_SCALE, AUG.GAUSSIAN_BLUR: augment.aug_settings(config, colour=True)), the per-image records of augment.colour_params travel
in the same header and color_hip.color_augment runs on resized_crop's uint8 result, on the same stream.  img and tok are device
tensors; index (int64 [B], the batch's positions in `items`) stays on the host, where the order was made.
"""
import concurrent.futures as cf
import os

import torch

from . import augment, color_hip, input_hip
from ._decode_worker import load_source
from .zeroshot import effective_cores, normalise_lut

CONTEXT = 77


def read_pairs(manifest, root=""):
    """`relative/path<TAB>caption` per line (UTF-8; empty lines are skipped, a caption may hold further tabs)
    -> [(os.path.join(root, path), caption)]."""
    items = []
    with open(manifest, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            path, tab, caption = line.partition("\t")
            if not tab or not path:
                raise ValueError(f"{manifest}:{n}: expected 'path<TAB>caption', got {line[:80]!r}")
            items.append((os.path.join(root, path), caption))
    return items


def _up(n, a):
    return (n + a - 1) // a * a


class PairPipeline:
    """settings: augment.aug_settings(config).  `slot`: the side of a staging slot = the largest side a decoded image keeps
    (load_source's max_side); at most MSCLIP_CROP_MAX_SCALE times the training size.  rank / world: this process's share of every
    epoch (augment.epoch_order); an epoch is whole batches only.  After a batch has been yielded, last_dims / last_boxes /
    last_flip are host tensors that describe it, and with a colour stage on so are last_ops / last_coef (augment.colour_params)."""

    def __init__(self, items, batch_size, device, settings, tokenizer=None, seed=0, workers=None, depth=3, slot=512, rank=0, world=1):
        self.items, self.bs, self.dev = list(items), int(batch_size), torch.device(device)
        self.settings, self.size, self.slot = dict(settings), int(settings["size"]), int(slot)
        if self.slot > input_hip.CROP_MAX_SCALE * self.size:
            raise ValueError(f"slot = {slot}: more than {input_hip.CROP_MAX_SCALE} times the training size {self.size}")
        if tokenizer is None:
            from .tokenizer import SimpleTokenizer
            tokenizer = SimpleTokenizer()
        self.tokenizer = tokenizer
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.workers = max(1, min(16, effective_cores()) if workers is None else int(workers))
        self.depth = max(2, int(depth))
        self.pool = cf.ThreadPoolExecutor(self.workers)
        B, S = self.bs, self.slot
        # the colour stages that are on (msclip_color_augment's mask); 0: the pipeline draws, stages and launches what it did without
        self.stages = augment.colour_stages(self.settings)
        # one staging buffer: tokens int64 [B, 77] | dims int32 [B, 2] | boxes int32 [B, 4] | flip int32 [B] | with a colour stage
        # on: ops int32 [B, 8] | coef fp32 [B, 12] | pad | pixels [B, S, S, 3]
        self.o_dims = B * CONTEXT * 8
        self.o_boxes = self.o_dims + B * 8
        self.o_flip = self.o_boxes + B * 16
        self.o_ops = self.o_flip + B * 4
        self.o_coef = self.o_ops + (B * 4 * color_hip.OPS if self.stages else 0)
        self.o_pix = _up(self.o_coef + (B * 4 * color_hip.COEF if self.stages else 0), 256)
        nbytes = self.o_pix + B * S * S * 3
        self.pin = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self.gpu = [torch.empty(nbytes, dtype=torch.uint8, device=self.dev) for _ in range(self.depth)]
        self.pin_v = [self._views(t) for t in self.pin]
        # what the workers write through: numpy views of the pinned buffers (a strided torch copy_ would start an intra-op thread
        # team per worker thread: 16 workers x 16 threads on 16 cores)
        self.pin_np = [{k: v[k].numpy() for k in ("pix", "tok")} for v in self.pin_v]
        self.gpu_v = [self._views(t) for t in self.gpu]
        self.free = [torch.cuda.Event() for _ in range(self.depth)]          # "the consumer is done with gpu[k]"
        self.copied = [None] * self.depth                                      # "the H2D copy out of pin[k] is done"
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.lut = normalise_lut(settings["mean"], settings["std"]).to(self.dev).contiguous()
        self.gen = torch.Generator()
        self.last_dims = self.last_boxes = self.last_flip = self.last_ops = self.last_coef = None
        self.epoch = self.pos = 0
        self.set_epoch(0)

    def _views(self, t):
        B, S = self.bs, self.slot
        v = dict(tok=t[:self.o_dims].view(torch.int64).view(B, CONTEXT), dims=t[self.o_dims:self.o_boxes].view(torch.int32).view(B, 2),
                 boxes=t[self.o_boxes:self.o_flip].view(torch.int32).view(B, 4),
                 flip=t[self.o_flip:self.o_flip + B * 4].view(torch.int32), pix=t[self.o_pix:].view(B, S, S, 3))
        if self.stages:
            v["ops"] = t[self.o_ops:self.o_coef].view(torch.int32).view(B, color_hip.OPS)
            v["coef"] = t[self.o_coef:self.o_coef + B * 4 * color_hip.COEF].view(torch.float32).view(B, color_hip.COEF)
        return v

    # ---- the epoch, the position in it and the generator: what a resumed pipeline needs
    def set_epoch(self, epoch):
        """Select `epoch` from its start: its order (seed, epoch) and a generator seeded from (seed, epoch).  The rank is NOT in the
        generator's seed, on purpose: every rank draws the same uniforms for slot j of batch b (on different images, so the same
        relative box and the same flip flag), which makes one saved state (rank 0's sidecar file) valid for every rank."""
        self.epoch, self.pos = int(epoch), 0
        self.order = augment.epoch_order(len(self.items), self.epoch, self.seed, self.rank, self.world, self.bs)
        self.gen.manual_seed((self.seed * 1000003 + self.epoch * 7919 + 17) % (2 ** 63))

    def __len__(self):
        return int(self.order.shape[0])

    def state_dict(self):
        return {"epoch": self.epoch, "pos": self.pos, "seed": self.seed, "rng_state": self.gen.get_state().clone(),
                "world": self.world, "batch_size": self.bs, "n": len(self.items)}

    def load_state_dict(self, state):
        for key, mine in (("world", self.world), ("batch_size", self.bs), ("n", len(self.items))):    # (the same on every rank)
            if state[key] != mine:
                raise ValueError(f"PairPipeline: the state was taken with {key} = {state[key]}, this pipeline has {mine}")
        self.seed = int(state["seed"])
        self.set_epoch(state["epoch"])
        self.pos = int(state["pos"])
        self.gen.set_state(state["rng_state"])

    # ---- workers
    def _decode_into(self, k, j, path):
        a = load_source(path, self.slot)
        h, w = a.shape[:2]
        self.pin_np[k]["pix"][j, :h, :w] = a
        return h, w

    def _tokenize_into(self, k, captions):
        # ONE task per batch: the tokenizer is pure Python, and a caption per decoding task put every worker in the queue for the
        # interpreter
        self.pin_np[k]["tok"][:] = self.tokenizer(captions).numpy()

    def _submit(self, b):
        k = b % self.depth
        if self.copied[k] is not None:
            self.copied[k].synchronize()                 # the HOST waits: pin[k]'s previous batch has left it before a worker writes
        idx = self.order[b]
        chunk = [self.items[int(i)] for i in idx]
        futs = [self.pool.submit(self._decode_into, k, j, path) for j, (path, _) in enumerate(chunk)]
        return idx, futs, self.pool.submit(self._tokenize_into, k, [c for _, c in chunk])

    def __iter__(self):
        nb, start = len(self), self.pos
        inflight = {b: self._submit(b) for b in range(start, min(start + self.depth - 1, nb))}
        try:
            for b in range(start, nb):
                idx, futs, tokfut = inflight.pop(b)
                k = b % self.depth
                sizes = torch.tensor([f.result() for f in futs], dtype=torch.int64)        # (re-raises a decoding error)
                tokfut.result()
                # draws in batch order from the pipeline's generator; the boxes on the host, nothing read back from the device
                u = torch.rand(self.bs, augment.ATTEMPTS, 4, dtype=torch.float64, generator=self.gen)
                uf = torch.rand(self.bs, dtype=torch.float64, generator=self.gen)
                boxes = augment.random_resized_crop_boxes(sizes, u, self.settings["scale"], self.settings["ratio"])
                flip = (uf < self.settings["flip_prob"]).to(torch.int32)
                pv, gv = self.pin_v[k], self.gpu_v[k]
                pv["dims"].copy_(sizes.to(torch.int32))
                pv["boxes"].copy_(boxes)
                pv["flip"].copy_(flip)
                ops = coef = None
                if self.stages:                          # (after the flip uniforms: with every colour stage off, the draws of before)
                    uc = torch.rand(self.bs, augment.COLOUR_DRAWS, dtype=torch.float64, generator=self.gen)
                    ops, coef = augment.colour_params(uc, self.settings)
                    pv["ops"].copy_(ops)
                    pv["coef"].copy_(coef)
                cur = torch.cuda.current_stream(self.dev)
                with torch.cuda.stream(self.copy_stream):
                    self.copy_stream.wait_event(self.free[k])        # gpu[k]'s previous batch has been consumed
                    self.gpu[k].copy_(self.pin[k], non_blocking=True)
                    landed = torch.cuda.Event()
                    landed.record(self.copy_stream)
                self.copied[k] = landed
                nxt = b + self.depth - 1
                if nxt < nb:
                    inflight[nxt] = self._submit(nxt)
                cur.wait_event(landed)
                if self.stages:
                    # (msclip_resized_crop requires an `out`: its fp32 result is written, then overwritten by the colour stage)
                    img, u8 = input_hip.resized_crop(gv["pix"], gv["dims"], gv["boxes"], self.lut, self.size, flip=gv["flip"],
                                                     filter=self.settings["interpolation"], want_u8=True)
                    color_hip.color_augment(u8, gv["ops"], gv["coef"], self.lut, stages=self.stages, out=img)
                else:
                    img = input_hip.resized_crop(gv["pix"], gv["dims"], gv["boxes"], self.lut, self.size, flip=gv["flip"],
                                                 filter=self.settings["interpolation"])
                tok = gv["tok"].clone()
                self.free[k].record(cur)
                self.last_dims, self.last_boxes, self.last_flip = sizes.to(torch.int32), boxes, flip
                self.last_ops, self.last_coef = ops, coef
                self.pos = b + 1
                yield img, tok, idx
        finally:
            for _, futs, tokfut in inflight.values():    # an abandoned iteration: no worker is left writing a staging buffer
                for f in futs + [tokfut]:
                    f.cancel()
                cf.wait(futs + [tokfut])

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
        for ev in self.copied:
            if ev is not None:
                ev.synchronize()
