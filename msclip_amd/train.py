"""Training step of the MS-CLIP-S hot path: forward that keeps what the backward needs, backward of every parameter,
AdamW.

The reference release contains no trainer and no loss; what is differentiated here is the forward it defines
(lib/models/clip_openai_pe_res_v1.py, "M.py") and the symmetric cross-entropy this build adds, with the reference's
gather semantics (gradient only through the local rows, lib/utils/comm.py:151-152) and its optimizer hyper-parameters
(separate LR / weight decay for the shared tensors: experiments/model/*-msclips.yaml `LR_SHARE` / `WD_SHARE`, scaled
with the world size in lib/config/default.py:299-304; no decay on bias / LayerNorm / BatchNorm, `WITHOUT_WD_LIST`).

This file: the token side -- the contrastive head (fused LSE sweeps forward; dL/dlogits blocks + GEMMs backward), L2
norm, both projections, ln_post / ln_final; all transformer blocks of both towers (LayerNorm, QKV / out_proj / c_fc /
c_proj dgrad + wgrad through msclip_gemm, msclip_attention_bwd, QuickGELU), where the modality-shared tensors
(M.py:2808-2830) receive the SUM of the image- and text-row gradients because the towers' tokens are rows of one matrix
and one wgrad GEMM contracts over all of them; the token path of the lateral adapters, ln_pre, class / positional /
token embeddings; the AdamW step and the rank averaging (comm.GradReducer).  train_conv.py: the convolutional side
(stem, parallel branch, adapter convolutions) with train-mode BatchNorm (bn="batch": per-GPU batch statistics, running
statistics updated) or frozen statistics (bn="frozen").  Together: all 325 gradient tensors of both released configs.
The patch-conv ViT-L/14 (BASELINE config C5, 257-token grid; bf16 only) has no conv side: its 406 gradient tensors are the
token side's plus the patch weight's (_patch_wgrad), and bn is moot there (no BatchNorm layer).

Parity: tests/test_gpu_train.py compares every gradient with autograd of the REAL reference
(tests/golden/*.grads.npz in eval() mode, b32-yfcc-msclips.grads_trainbn.npz in train() mode; captured by
tools/make_golden.py::grads_fixture); the L/14 in tests/test_gpu_train_l14.py (l14-fp8-msclips.grads.npz).
"""

import torch
import torch.distributed as dist

from . import comm as C
from . import hip
from . import gradgemm
from . import options
from .engine import Captions
from .gradgemm import dgrad as _dgrad, wgrad as _wgrad, wgrad_async as _wgrad_async
from .train_conv import ConvSideBackward, ConvSideBatchNorm

BF = torch.bfloat16
F32 = torch.float32
DROP_PATH_MODES = ("sample", "position")
_LEAVES = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
           "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


OPTIMIZERS = {"adamw": 1e-8, "lamb": 1e-6}              # TrainStep(optimizer=...): the default eps of each
NONFINITE = (None, "skip", "raise")                     # TrainStep(nonfinite=...)


class TrainStep:
    """forward + backward (+ AdamW step) for one local batch.  `engine` is the model's msclip_amd.engine.Engine."""

    def __init__(self, model, lr=None, lr_share=None, wd=0.05, wd_share=None, betas=(0.9, 0.999), eps=None, bn="frozen",
                 without_wd=("bn", "bias", "ln"), clip_grad_norm=None, ema_decay=None, drop_path=None, drop_path_mode="sample",
                 drop_path_seed=0, optimizer="adamw", trust_clip=False, always_adapt=False, nonfinite=None):
        """bn = "frozen": BatchNorm with its running statistics (gamma / beta trained; the inference kernels' folded
        form); bn = "batch": train-mode BatchNorm -- per-GPU batch statistics in the forward, their backward, running
        statistics updated with momentum 0.1 (what the reference's modules do in train()).
        Optimizer defaults are the reference yaml's (experiments/model/b32.yaml:39-50: adamW, WD 0.05, no decay on
        'bn' / 'bias' / 'ln'; no OPTIMIZER_ARGS => torch.optim.AdamW's betas (0.9, 0.999) and eps 1e-8).
        `without_wd`: TRAIN.WITHOUT_WD_LIST keywords ('bn': BatchNorm parameters, 'ln': LayerNorm parameters, 'bias': names
        ending in 'bias').
        `clip_grad_norm`: TRAIN.CLIP_GRAD_NORM, the max_norm of torch.nn.utils.clip_grad_norm_ applied inside step(); None, 0
        and 0.0 mean no clipping (the reference's default, lib/config/default.py:153).
        `ema_decay`: TRAIN.EMA_DECAY in [0, 1): fp32 shadow weights (self.ema_shadow, one per entry of named_parameters(),
        buffers not included) that start as copies of the parameters and follow them on the device after every step(),
        shadow = decay * shadow + (1 - decay) * parameter; ema_assign() / ema_resume() / ema_weights() put them into the model
        for evaluation and saving.  None, 0 and 0.0 mean no EMA (the reference's default, lib/config/default.py:146).
        `drop_path`: MODEL.SPEC.VISION.DROP_PATH in [0, 1), stochastic depth on both residual branches of every vision block
        (timm's DropPath, M.py:801, 1027-1028; the text blocks have none); None takes model.drop_path (what get_clip_model read
        from the config), 0 / 0.0 switch it off whatever the model says.  `drop_path_mode`: "sample" = one Bernoulli(1 - p) draw
        per image per branch (what stochastic depth means); "position" = one draw per token position per branch, shared by all
        images -- what the reference module computes, because its blocks run sequence-first and timm draws per index of
        dimension 0.  The masks come from a device torch.Generator seeded with `drop_path_seed` (no host
        synchronisation; its state travels in the checkpoint); forward() leaves them in self.last_drop_masks and replays given
        ones (drop_masks=...).  Off, the step issues exactly the launches it issued before the option existed.
        `optimizer`: "adamw" or "lamb" (TRAIN.OPTIMIZER, case-insensitive).  lamb is timm's Lamb: the AdamW update with each
        parameter tensor's rate scaled by its trust ratio ||w|| / ||u|| where its weight decay is not 0 (everywhere with
        `always_adapt`), capped at 1 with `trust_clip`; step() describes it.  `eps`: None takes the optimizer's default, 1e-8
        for adamw (torch.optim.AdamW's), 1e-6 for lamb (timm's).
        `nonfinite`: None (default): a NaN or Inf in the gradients reaches the parameters, as it does in torch, and step() is
        what it was before the option existed.  "skip" (TRAIN.SKIP_NONFINITE): step() leaves parameters, moments and the
        engine's packed copies untouched when any gradient element is NaN or Inf -- decided on the device, nothing read back
        in the step -- and the bias corrections count applied updates only (step() says how).  "raise"
        (TRAIN.DETECT_ANOMALY): "skip", then step() reads the verdict and raises FloatingPointError naming the gradient
        tensors; model and optimizer state are intact when it does."""
        assert bn in ("frozen", "batch")
        if nonfinite not in NONFINITE:
            raise ValueError(f"nonfinite = {nonfinite!r}: one of {NONFINITE}")
        self.nonfinite = nonfinite
        self.last_skipped = None
        self._skip_base = 0                  # skipped steps counted by earlier optimizer tables / a resumed checkpoint
        self._skip_seen = 0                  # ... and by the current table, as of the last verdict that arrived
        self._skip_host = self._skip_event = None      # pinned int32 pair <- guard_state[0:2] of the last step(), its event
        optimizer = str(optimizer).lower()
        if optimizer not in OPTIMIZERS:
            raise NotImplementedError(f"optimizer = {optimizer!r}: one of {OPTIMIZERS}")
        self.optimizer, self.trust_clip, self.always_adapt = optimizer, bool(trust_clip), bool(always_adapt)
        self._run_options = {"trust_clip": self.trust_clip} if optimizer == "lamb" else {}      # of the optimizer table's run()
        if eps is None:
            eps = OPTIMIZERS[optimizer]
        self.last_trust_ratio = self.last_param_norm = self.last_update_norm = None
        if drop_path is None:
            drop_path = getattr(model, "drop_path", 0.0)
        if not 0.0 <= float(drop_path or 0.0) < 1.0:
            raise ValueError(f"drop_path = {drop_path!r}: a drop rate in [0, 1) (or None for the model's, 0 for none)")
        if drop_path_mode not in DROP_PATH_MODES:
            raise ValueError(f"drop_path_mode = {drop_path_mode!r}: one of {DROP_PATH_MODES}")
        self.drop_path = float(drop_path or 0.0)
        self.drop_path_mode, self.drop_path_seed = drop_path_mode, int(drop_path_seed)
        self.last_drop_masks = None
        if clip_grad_norm is not None and not float(clip_grad_norm) >= 0.0:
            raise ValueError(f"clip_grad_norm = {clip_grad_norm!r}: a max_norm >= 0 (or None / 0 for no clipping)")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay = {ema_decay!r}: a decay in [0, 1) (or None / 0 for no EMA)")
        self.ema_decay = float(ema_decay) if ema_decay else None
        self.clip_grad_norm = clip_grad_norm
        self.last_grad_norm = self.last_clip_coef = None
        unknown = set(without_wd) - {"bn", "bias", "ln", "gn", "dw"}
        if unknown:
            raise NotImplementedError(f"TRAIN.WITHOUT_WD_LIST keywords {sorted(unknown)} are not implemented")
        self.without_wd = tuple(without_wd)
        self.bn = bn
        self.convbn = None
        self.model = model
        self.eng = model.engine()
        self.dev = self.eng.dev
        if self.eng.patch and self.eng.fp8:
            raise NotImplementedError("TrainStep trains the patch-conv (ViT-L/14) model in bf16 only: build it with "
                                      "MODEL.SPEC.PRECISION bf16 (fp8 training is not implemented)")
        self.lr, self.lr_share = lr, lr_share
        self.wd, self.wd_share = wd, wd_share
        self.betas, self.eps = betas, eps
        self.state = {}
        self.steps = 0
        self._ema = _EmaShadow(model) if self.ema_decay else None
        self.ema_shadow = self._ema.views if self._ema else None      # {name: fp32 view of the arena}, named_parameters() order
        self.ema_updates = 0
        self._ema_assigned = False
        self._ema_conv_pack = None           # the engine's conv_pack kind at ema_assign(): ema_resume() repeats a table re-pack
        self.saved = None                    # activations of a forward() that backward() has not consumed yet
        self.reducer = None                  # comm.GradReducer of the last backward() (None at world size 1)
        self._plan = None                    # the optimizer launch's tensor table (_adamw_plan)
        self._acc = None                     # accumulate()'s persistent gradient accumulators (_Accumulators)
        self._wt_plan = None                 # hip.TransposePlan of the backward's W^T operands
        self.schedule = None                 # learning-rate schedule (from_config sets it; set_epoch applies it)
        self._base_lr = None                 # (lr, lr_share) before the schedule first touched them
        self.phase_events = None             # tools/accumulate_bench.py sets []: _mark() appends (name, timing event)
        self._dp_gen = None
        if self.drop_path:
            self._dp_gen = torch.Generator(device=self.dev)
            self._dp_gen.manual_seed(self.drop_path_seed)

    # ------------------------------------------------------------------ stochastic depth: masks
    def drop_mask_shape(self, Bi):
        """Shape of one set of keep masks for a batch of Bi images: [vision blocks that run, 2 (attention, MLP branch), Bi]
        in "sample" mode, [.., 2, tokens per image] in "position" mode."""
        e = self.eng
        return (sum(b is not None for b in e.vblk), 2, Bi if self.drop_path_mode == "sample" else e.Lv)

    def draw_drop_masks(self, Bi):
        """One set of keep masks (bool, on the device) from this TrainStep's generator: True with probability 1 - drop_path,
        every entry independent.  Queued on the current stream; nothing visits the host."""
        if self._dp_gen is None:
            raise RuntimeError("TrainStep.draw_drop_masks() needs drop_path > 0")
        return torch.rand(self.drop_mask_shape(Bi), generator=self._dp_gen, device=self.dev) < (1.0 - self.drop_path)

    def _check_drop_masks(self, masks, Bi):
        if masks.dtype != torch.bool or tuple(masks.shape) != self.drop_mask_shape(Bi):
            raise ValueError(f"drop_masks: a bool tensor of shape {self.drop_mask_shape(Bi)} in {self.drop_path_mode!r} mode, got "
                             f"{masks.dtype} {tuple(masks.shape)}")
        return masks.to(self.dev)

    # ------------------------------------------------------------------ forward that keeps what the backward needs
    @hip.off_default_stream
    def forward(self, img, tok, drop_masks=None, _head=True, _update_stats=True):
        """drop_masks: replay these keep masks (drop_mask_shape(batch), bool) instead of drawing a set -- also with
        drop_path 0, where kept rows then carry the scale 1.0 exactly.  The masks used are left in self.last_drop_masks
        (None when the step runs without stochastic depth).
        _head=False (accumulate() only): stop in front of the contrastive head and return the two gather payloads; the saved
        activations then wait for a backward(_dfeat=...).  _update_stats=False: train-mode BatchNorm normalises with the
        batch statistics but leaves the module's running statistics alone (accumulate()'s feature pass)."""
        self._ema_live("forward")
        e = self.eng
        e.refresh()
        with torch.cuda.device(e.dev), torch.no_grad():
            sv = self._begin_forward(img, tok, drop_masks)
            w, Bi, drop_masks = sv["w"], sv["Bi"], self.last_drop_masks
            cb, conv_events = self._conv_side_forward(sv)
            M = sv["M"] = w["M"]
            sv.update(Lmax=w["Lmax"], pad=w["pad"], Mt_live=w["Mt_live"])
            # stochastic depth: the row-scale tables of every vision block's two branches, [blocks, 2, M] fp32 (image rows 0 or
            # 1 / keep, text rows 1); the out_proj / c_proj launches of the vision rows carry their slice, the backward reads
            # the slices saved with the layer (None: the option is off and nothing below changes)
            dp_tab = None if drop_masks is None else drop_path_table(drop_masks, Bi, e.Lv, M, self.drop_path_mode, 1.0 - self.drop_path)
            dp_next = 0
            e._text_front(sv["tok"], w, sv["Bt"])
            # ---- blocks.  Xc = the residual matrix the next layer reads: the workspace's X at first; every layer that runs over
            # all rows writes its two residual updates into fresh matrices (the backward needs the layer's input and its
            # post-attention state: they stay where they are instead of being cloned), so Xc moves on.
            Xc = w["X"]
            for i in range(e.n_layers):
                L = dict(adapter=None, rs=None)
                if e.vblk[i] is not None and dp_tab is not None:
                    L["rs"] = (dp_tab[dp_next, 0], dp_tab[dp_next, 1])          # (attention branch, MLP branch), each fp32 [M]
                    dp_next += 1
                if e.vblk[i] is not None and i in e.lateral:
                    self._adapter_forward(sv, L, i, Xc, cb, conv_events)
                Xc = self._block_forward(sv, L, i, Xc)
            pi, pt = self._features(sv, Xc, cb, _update_stats)
            loss = self._contrastive_loss(sv, pi, pt) if _head else None
            self.saved = sv
            return loss if _head else (pi, pt)

    def _begin_forward(self, img, tok, drop_masks):
        """The checks, the masks, the held workspace, the captions' staging / packing -> sv, the dict of what backward() reads."""
        e = self.eng
        Bi, Bt = img.shape[0], tok.shape[0]
        assert Bi == Bt, "a training step needs image-text pairs"
        if drop_masks is not None:
            drop_masks = self._check_drop_masks(drop_masks, Bi)
        elif self.drop_path:
            drop_masks = self.draw_drop_masks(Bi)
        self.last_drop_masks = drop_masks
        if e.Lv > hip.ATTENTION_BWD_MAX_L or e.Lt > hip.ATTENTION_BWD_MAX_L:
            raise NotImplementedError(f"msclip_attention_bwd covers sequences up to {hip.ATTENTION_BWD_MAX_L} tokens")
        self._release_saved()                                  # a forward that was never differentiated: release its maps
        w = e._workspace(Bi, Bt)
        # the conv side's maps (w["stem"], w["par"], w["pool"], S1, P0) -- or the patch-conv model's patch matrix
        # w["PATCH"] -- are read again by backward(): until then the engine's inference entry points (an eval / logging
        # call of the same shape in between) get another workspace
        w["held"] = True
        # captions run packed like the inference path (engine.text_pack_enabled): rows behind a caption's EOT position
        # neither influence an output nor receive a gradient.  `tok` may be a batch staged ahead (engine.stage_captions).
        pack = e.text_pack_enabled()
        cap = tok if isinstance(tok, Captions) else None
        tokc = cap.tok if cap is not None else e._check_tok(tok)
        if pack and cap is None:
            cap = e.stage_captions(tokc)
        if not pack:
            cap = None
            e._text_unpacked(w, Bt)
        else:
            e._text_sizes(cap, w, Bt)                   # the host read (immediate for a batch staged a step ahead)
        sv = dict(Bi=Bi, Bt=Bt, Mv=w["Mv"], layers=[None] * e.n_layers, tok=tokc, w=w, cap=cap)
        sv["img"] = e._check_img(img)
        return sv

    def _conv_side_forward(self, sv):
        """The fronts (the conv side's maps stay in the workspace `w`; the tokens in front of ln_pre are cloned) and the side
        stream's share of the conv side -> (the train-mode BatchNorm object or None, the adapters' events or None)."""
        e, w, Bi = self.eng, sv["w"], sv["Bi"]
        keep = []
        cb = None
        if self.bn == "batch" and not e.patch:             # (the patch-conv model has no BatchNorm: bn is moot there)
            if self.convbn is None:
                self.convbn = ConvSideBatchNorm(self)
            cb = self.convbn
            cb.begin(sv["img"], w, Bi)
            cb.front()
        # unfused=True at every engine call: the conv side runs layer by layer, every map the backward reads stays in `w`
        e._vision_front(sv["img"], w, Bi, keep_pre=keep, convs_done=cb is not None, unfused=True)
        sv["tok_pre"] = keep[0]
        # frozen statistics: the image-only conv branch + the adapters' top-down halves on the engine's side stream, as in
        # the inference schedule (same-box A/B: 89.6-90.2 -> 88.5-88.9 ms per step)
        conv_events = None
        side_ok = not e.patch and gradgemm.lane_enabled() and e.lateral == sorted(e.lateral)
        if side_ok and cb is None:
            conv_events = e._conv_branch_on_side_stream(w, Bi, unfused=True)
        elif side_ok:
            # train-mode BatchNorm: the same for the raw-conv -> statistics -> normalise chains of the parallel branch and
            # the adapters' top-down halves (they depend on the image only)
            if w["Ts"] is None:
                w["Ts"] = [torch.empty(Bi * e.g * e.g, e.D, dtype=F32, device=e.dev) for _ in e.adapters]
            side = C.side_stream(e.dev)
            conv_events = []
            mine = set(cb.saved)
            with hip.forked(side) as cur_s:
                for j in range(len(e.adapters)):
                    cb.stage(j)
                    cb.adapter_top(j, w["Ts"][j])
                    ev = torch.cuda.Event()
                    ev.record(side)
                    conv_events.append(ev)
            # the raw maps and statistics made there come from the side stream's pool; the backward and the running-statistics
            # update read them on this stream (behind conv_events), which the allocator has to know before they are freed
            cb.record_stream(cur_s, skip=mine)
        return cb, conv_events

    def _adapter_forward(self, sv, L, i, Xc, cb, conv_events):
        """Lateral adapter in front of block i, X[:Mv] <- ln_adapt(token path + top-down map); L["adapter"]: what its backward reads."""
        e, w, Bi, Mv = self.eng, sv["w"], sv["Bi"], sv["Mv"]
        j = e.lateral.index(i)
        a = e.adapters[j]
        asum = torch.empty(Mv, e.D, dtype=F32, device=e.dev)
        if cb is not None and conv_events is not None:
            torch.cuda.current_stream(e.dev).wait_event(conv_events[j])
            cb.adapter_sum(j, Xc[:Mv], w["Ts"][j], asum)
        elif cb is not None:
            cb.stage(j)
            cb.adapter_top(j, w["T"])
            cb.adapter_sum(j, Xc[:Mv], w["T"], asum)
        elif conv_events is not None:
            torch.cuda.current_stream(e.dev).wait_event(conv_events[j])
            hip.adapter_sum(Xc[:Mv], w["Ts"][j], a["dww"], a["dwb"], asum, Bi, e.Lv, e.g, e.usecls)
        else:
            e._parallel_stage(j, w, Bi, unfused=True)
            hip.dwpool(w["par"][j], a["pool"], w["pool"][j], Bi, e.par_hw[j], e.par_hw[j], a["C"], a["k"])
            hip.gemm(w["pool"][j], a["pw"].weight, w["T"], M=Bi * e.g * e.g, N=a["pw"].cout, bias=a["pw"].bias, ldx=a["pw"].cin)
            hip.adapter_sum(Xc[:Mv], w["T"], a["dww"], a["dwb"], asum, Bi, e.Lv, e.g, e.usecls)
        x_pre = Xc[:Mv].clone()                                                   # what the depthwise 3x3 read
        hip.layernorm(asum, a["ln"].g, a["ln"].b, Xc[:Mv], Mv)                    # X[:Mv] <- ln_adapt(sum), fp32
        L["adapter"] = dict(j=j, sum=asum, x_pre=x_pre)

    def _block_forward(self, sv, L, i, Xc):
        """Block i of both towers over the token matrix Xc -> the next block's; sv["layers"][i] = L, what its backward reads."""
        e, w, Bi, Bt, Mv, M = self.eng, sv["w"], sv["Bi"], sv["Bt"], sv["Mv"], sv["M"]
        D, dev = e.D, e.dev
        vb, tb = e.vblk[i], e.tblk[i]
        segs = ([(0, Mv, vb)] if vb is not None else []) + [(Mv, M, tb)]
        r_lo = segs[0][0]
        fresh = r_lo == 0                         # (text block 0 leaves the image rows alone: in place, cloned)
        L["x_in"] = Xc if fresh else Xc[r_lo:M].clone()
        # Round 6: behind the LAST block only x[:, 0] of every image (M.py:2685) and the EOT row of every caption (M.py:3057-3060)
        # are read, and out_proj / ln_2 / c_fc / c_proj are row-wise: they run -- forward here, backward in backward() -- on
        # those Bi + Bt rows instead of on every token (what the inference path has done since round 3; the rows' gradients
        # are the only non-zero ones behind the block, so every parameter gradient is unchanged)
        compact = (i == e.n_layers - 1 and len(segs) == 2 and L["adapter"] is None and options.TRAIN.compact_last_block)
        XM = None if compact else (torch.empty(M, D, dtype=F32, device=dev) if fresh else Xc)
        lno1 = torch.empty(M, D, dtype=BF, device=dev)
        e._layernorm(segs, "ln1", Xc, lno1)        # (both towers' rows in one launch, modality-specific gamma / beta)
        groups = e._groups(segs)
        qkv = torch.empty(M, 3 * D, dtype=BF, device=dev)
        ao = torch.empty(M, D, dtype=BF, device=dev)
        for r0, r1, bw in groups:
            hip.gemm(lno1[r0:r1], bw.wqkv, qkv[r0:r1], bias=bw.bqkv)
        if vb is not None:
            hip.attention(qkv[:Mv], ao[:Mv], Bi, e.Lv, e.heads, False)
        e._attention_text(w, qkv, ao, Bt)
        L.update(r_lo=r_lo, segs=segs, groups=groups, lno1=lno1, qkv=qkv, ao=ao)
        sv["layers"][i] = L
        if not compact:
            L["x_mid"], L["lno2"], L["h"], L["hid"], XN = self._tail_forward(Xc, ao, XM, segs, groups, L["rs"], Mv, True)
            return XN
        nc = Bi + Bt
        crow = torch.cat([torch.arange(0, Mv, e.Lv, dtype=torch.int32, device=dev), w["eot"][:Bt]])   # live rows of X
        xin_c, ao_c = torch.empty(nc, D, dtype=F32, device=dev), torch.empty(nc, D, dtype=BF, device=dev)
        hip.gather_rows(Xc, xin_c, nc, row_idx=crow)
        hip.gather_rows(ao, ao_c, nc, row_idx=crow)
        csegs = e._live_segs(Bi, Bt, vb, tb)
        cgroups = e._groups(csegs)
        xm_c = torch.empty(nc, D, dtype=F32, device=dev)
        # the compact rows' scales: the table gathered with the same row list as the activations ([2, nc]; a few KB)
        rs_c = None if L["rs"] is None else torch.stack(L["rs"]).index_select(1, crow.long()).contiguous()
        xm_c, lno2_c, h_c, hid_c, xn_c = self._tail_forward(xin_c, ao_c, xm_c, csegs, cgroups, rs_c, Bi, False)
        L["compact"] = dict(crow=crow, cgroups=cgroups, ao=ao_c, x_mid=xm_c, lno2=lno2_c, h=h_c, hid=hid_c, x_out=xn_c, rs=rs_c)
        sv["compact"] = xn_c
        return Xc

    def _tail_forward(self, x_in, ao, x_mid, segs, groups, rs, first_row_of_text, fuse_act):
        """The block's row-wise tail over whatever rows it is given (all tokens, or the last block's live rows): out_proj + residual
        -> x_mid (the caller's matrix; x_in itself where the block runs in place), ln_2, c_fc, QuickGELU, c_proj + residual
        -> (x_mid as the backward wants it, lno2, h, hid, x_out).  rs: the two branches' row scales, (attention, MLP) or [2, rows]
        (None: no stochastic depth).  fuse_act: the all-token call -- c_fc may write activation and pre-activation in one launch,
        and x_out is allocated in front of ln_2's output as that path always did; the live-row call always takes two launches
        (the two forms round h differently) and allocates x_out last."""
        e = self.eng
        D, dev, r_lo, n = e.D, e.dev, segs[0][0], segs[-1][1]
        for r0, r1, bw in groups:
            hip.gemm(ao[r0:r1], bw.wo, x_mid[r0:r1], bias=bw.bo, resid=x_in[r0:r1], resid_kind=hip.RESID_F32,
                     row_scale=_rs_rows(rs, 0, r0, r1, first_row_of_text))
        in_place = x_mid is x_in
        mid = x_mid[r_lo:n].clone() if in_place else x_mid
        x_out = x_in if in_place else (torch.empty(n, D, dtype=F32, device=dev) if fuse_act else None)
        lno2 = torch.empty(n, D, dtype=BF, device=dev)
        e._layernorm(segs, "ln2", x_mid, lno2)
        h = torch.empty(n, 4 * D, dtype=BF, device=dev)
        hid = torch.empty(n, 4 * D, dtype=BF, device=dev)
        if x_out is None:
            x_out = torch.empty(n, D, dtype=F32, device=dev)
        for r0, r1, bw in groups:
            if fuse_act and (r1 - r0) % 256 == 0:
                # ONE launch writes the pre-activation (the backward's QuickGELU' needs it) and the activation
                # (the ping-pong kernel's training forms cover whole 256-row tiles: any other row count takes two launches)
                hip.gemm(lno2[r0:r1], bw.wfc, hid[r0:r1], bias=bw.bfc, act=hip.ACT_QUICKGELU, out2=h[r0:r1])
            else:
                hip.gemm(lno2[r0:r1], bw.wfc, h[r0:r1], bias=bw.bfc)
                hip.quickgelu(h[r0:r1], hid[r0:r1])
        for r0, r1, bw in groups:
            hip.gemm(hid[r0:r1], bw.wpr, x_out[r0:r1], bias=bw.bpr, resid=x_mid[r0:r1], resid_kind=hip.RESID_F32,
                     row_scale=_rs_rows(rs, 1, r0, r1, first_row_of_text))
        return mid, lno2, h, hid, x_out

    def _features(self, sv, Xc, cb, _update_stats):
        """Heads, the copies the backward reads -> the gather payloads (pi, pt): bf16 hi | lo of the scaled image / the text features."""
        e, w, Bi, Bt, M = self.eng, sv["w"], sv["Bi"], sv["Bt"], sv["M"]
        X = w["X"]
        if cb is not None and _update_stats:
            cb.update_running_stats()
        # ---- heads + loss
        if sv.get("compact") is not None:
            # the heads read the compact matrix of the last block's live rows (image cls rows, then EOT rows)
            sv["x_out"] = sv["compact"]
            e._head_image(w, Bi, compact=True, x=sv["compact"])
            e._head_text(w, Bt, compact=True, Bi=Bi, x=sv["compact"])
        else:
            sv["x_out"] = Xc if Xc is not X else X[:M].clone()
            e._head_image(w, Bi, x=Xc)               # the heads read the final residual matrix
            e._head_text(w, Bt, x=Xc)
        sv.update(hv=w["hv"].clone(), ht=w["ht"].clone(), fv_raw=w["fv_raw"].clone(), ft_raw=w["ft_raw"].clone(),
                  fv=w["fv"].clone(), ft=w["ft"].clone(), fvb=w["fvb"].clone(), ftb=w["ftb"].clone(), eot=w["eot"].clone())
        # exp(logit_scale) stays ON THE DEVICE here: as a host scalar (the GEMM's alpha) it would have to be read back after
        # the previous step's optimizer update, i.e. the host would wait at this point of every forward until the GPU
        # has finished the step before (measured: forward returned after 83 ms instead of 5 with a step queued) and
        # then enqueue the backward against a GPU that is already running.  The image features carry the scale instead.
        s_dev = e.model.logit_scale.detach().float().exp()
        sv["scale"] = s_dev
        return _split_hi_lo(sv["fv"] * s_dev), _split_hi_lo(sv["ft"])

    def _contrastive_loss(self, sv, pi, pt):
        """Symmetric cross-entropy of this rank's rows against all ranks' -> 0-d loss; what the head's backward reads goes into sv."""
        e, Bi = self.eng, sv["Bi"]
        if C.comm.collectives:
            allpi, hi_ = C.gather_rows_async(pi)
            allpt, ht_ = C.gather_rows_async(pt)
            hi_.wait(); ht_.wait()
        else:
            allpi, allpt = pi, pt
        E = e.E
        n = allpi.shape[0]
        off = C.local_label_offset(Bi) if n > Bi else 0
        sv["off"], sv["n"] = off, n
        sv["allI"], sv["allT"] = allpi[:, :E].contiguous(), allpt[:, :E].contiguous()     # hi parts: dgrad operands (allI scaled)
        S_i = _logits(*_logit_operands(pi, allpt, E))                                      # image rows (they carry the scale)
        S_t = _logits(*_logit_operands(pt, allpi, E))                                      # caption rows
        lse = torch.empty(2, Bi, dtype=F32, device=e.dev)
        out = torch.empty(1, dtype=F32, device=e.dev)
        _loss_partial(S_i, S_t, lse[0], lse[1], off, n, out)
        sv["coll"] = n > Bi or C.comm.collectives
        if sv["coll"]:
            dist.all_reduce(out)
            lse_flat = torch.empty((n // Bi) * 2, Bi, dtype=F32, device=e.dev)            # concatenated along dim 0: every backend's form
            dist.all_gather_into_tensor(lse_flat, lse.contiguous())
            lse_all = lse_flat.view(n // Bi, 2, Bi).permute(1, 0, 2).reshape(2, n).contiguous()   # rank-major global order
        else:
            lse_all = lse
        sv.update(S_i=S_i, S_t=S_t, lse_loc=lse, lse_all=lse_all)
        return out[0].clone()

    # ------------------------------------------------------------------ backward
    @hip.off_default_stream
    def backward(self, reduce=True, bucket_bytes=64 << 20, clone=False, _dfeat=None):
        """-> {reference state_dict key: fp32 gradient} for every parameter of the slice (shared tensors under their
        visual.* key; the text-tower aliases are the same Parameter objects).  Under N > 1 ranks (and reduce=True) the
        gradients are averaged over the ranks as the reference's DDP wrapper would: every gradient goes into a
        comm.GradReducer bucket the moment it exists, and the buckets' RCCL all-reduces run on the side stream under
        the rest of the backward (last block's bucket first).
        LIFETIME: at world size > 1 the returned tensors are views into the per-device gradient-bucket arena, which the NEXT
        backward() on this device overwrites (in-place 1 / world scaling and split-K writes included): call step() before the
        next backward, or pass clone=True to own the tensors (gradient accumulation over micro-batches, comparing two backward
        passes, two TrainSteps on one device).  step() refuses stale views (comm.GradViews.check_fresh).  At world size 1 the
        gradients are fresh tensors either way.
        _dfeat (accumulate() only): (d loss / d image features, d loss / d text features, d loss / d logit_scale) of a
        forward that stopped in front of the head; the head's own backward is skipped, everything below it is the same."""
        e, sv = self.eng, self.saved
        if sv is None:
            raise RuntimeError("TrainStep.backward() needs the activations of a TrainStep.forward() that has not been "
                               "differentiated yet (call forward first; one backward per forward)")
        with torch.cuda.device(e.dev), torch.no_grad():
            reducer = C.GradReducer(bucket_bytes) if (reduce and C.comm.collectives) else None
            self.reducer = reducer
            bp = _BackwardPass(self, sv, reducer)
            bp.heads(_dfeat)
            bp.transposed_weights()
            # ---- blocks, last to first
            carry = None                      # (dY, bias sums) of this block's MLP half, left by the block above's ln_1 backward
            for i in reversed(range(e.n_layers)):
                L = sv["layers"][i]
                if L.get("compact") is not None:
                    assert carry is None
                    dlno, dao, dqkv = bp.compact_tail(i, L)
                else:
                    dlno, carry = bp.mlp(i, L, carry), None
                    dao, dqkv = bp.out_proj(i, L, dlno)
                qpart = bp.attention(i, L, dao, dqkv)
                bp.in_proj(i, L, dqkv, dlno, qpart)
                carry = bp.ln1_and_carry(i, L, dlno)
                if L["adapter"] is not None:
                    bp.adapter(i, L)
                sv["layers"][i] = None                                                         # free the layer's activations
                dlno = dao = dqkv = qpart = None             # (and its gradients: the next block allocates its own)
            dtok = bp.fronts()
            bp.folds.run()                                   # every deferred column sum of the transformer's backward, two launches
            if bp.conv is None:
                self._patch_wgrad(bp.grads, dtok, sv["w"]["PATCH"], sv["Bi"])
            else:
                bp.conv.stem(bp.grads, dtok)
            bp.flush_wgrads()
            gradgemm.join(e.dev)                                 # the gradients queued on the lane stream
            self._release_saved()
            return reducer.finish(clone=clone) if reducer is not None else dict(bp.grads)


    def _patch_wgrad(self, grads, dtok, patch, Bi):
        """visual.conv1.weight [D, 3, P, P] of the patch-conv stem (M.py:2657; kernel == stride == P, no bias): the forward was
        X[grid rows] = PATCH . W_patch^T over msclip_patchify's matrix (columns (c, kh, kw) in the weight's memory order, zero
        padding up to patch_k), so dW = dTok[grid rows]^T . PATCH -- the class rows skipped by the cast pass -- with the padding
        columns dropped."""
        e = self.eng
        g2, D, P = e.g * e.g, e.D, e.S // e.g
        kp = 3 * P * P
        dgrid = hip.cast_bf16_colsum(dtok[:Bi * e.Lv], fold=False, skip_group=g2)[0]      # grid rows, one pass, no gather copy
        grads["visual.conv1.weight"] = _wgrad_async(dgrid, patch[:Bi * g2], Bi * g2,
                                                    post=lambda d: d[:, :kp].reshape(D, 3, P, P).contiguous())

    # ------------------------------------------------------------------ exact large-batch step over chunks
    @hip.off_default_stream
    def accumulate(self, chunks, clone=False, check_features=False, drop_masks=None):
        """-> (loss, grads) of ONE contrastive batch made of all the chunks' pairs, computed one chunk at a time; follow it
        with step(grads).  chunks: a sequence indexed twice, K >= 1 pairs (img, tok), each acceptable to forward() (a staged
        engine.Captions included); chunk sizes may differ, N = sum of them.

        loss: the symmetric cross-entropy over all N pairs (0-d device tensor): the label of row i of chunk k is
        (sum of the earlier chunks' sizes) + i, the negatives are all N - 1 other pairs.  grads[key] = d loss / d parameter for
        every key backward() returns: the true gradient of that loss, no 1 / K factor.  A world of K ranks holding one chunk each
        would produce 1 / K of it (DDP's mean).  This is NOT the sum of K ordinary steps, whose pairs only compete with the
        negatives of their own chunk.

        bn="frozen": mathematically the one-shot step on the concatenated batch.  bn="batch": every chunk is normalised with
        its own batch statistics, as the K ranks of the reference would do; the running statistics are updated once per chunk,
        in chunk order, and end where K ordinary train-mode forward() calls over the same chunks leave them.

        Two passes (the only exact method that holds one chunk's activations at a time): (1) every chunk through the training
        forward's arithmetic, nothing kept, running statistics untouched: its gather payload (bf16 hi | lo of the scaled image
        features / of the text features) goes into a bank [N, 2E] per modality; (2) the head over the bank, one [B_k, N] row
        block at a time, with the one-shot step's kernels (its rank-sharded path, the bank in place of the all-gather): loss,
        both global LSE vectors, every chunk's feature gradients; (3) per chunk the saving forward, the backward below the head
        fed with those feature gradients, and msclip_grad_accumulate into the accumulators.  The features recomputed in (3)
        equal the banked ones bitwise (every kernel on the path is deterministic); check_features=True compares them and
        raises on the first chunk that differs.

        LIFETIME: the returned tensors are views of persistent fp32 accumulators owned by this TrainStep (stable addresses:
        the optimizer table is not rebuilt); they are valid until the next accumulate().  clone=True returns owned copies.
        K = 1 reproduces forward() + backward() bitwise (token_embedding.weight: atomic scatter-add, to rounding).

        Stochastic depth: ONE set of keep masks per chunk, drawn before the feature pass (chunk order) and used by both of the
        chunk's forwards -- the banked features and the differentiated ones belong to the same network.  drop_masks: a
        sequence of K mask tensors to replay instead (forward()'s drop_masks, per chunk); the sets used are left in
        self.last_drop_masks as a list."""
        if C.comm.collectives or C.comm.world_size > 1:
            raise NotImplementedError("TrainStep.accumulate() covers a single process: chunks composed with ranks (world size "
                                      f"{C.comm.world_size}) are not implemented")
        self._ema_live("accumulate")
        K = len(chunks)
        if K < 1:
            raise ValueError("TrainStep.accumulate() needs at least one (img, tok) chunk")
        if drop_masks is not None and len(drop_masks) != K:
            raise ValueError(f"TrainStep.accumulate(): {len(drop_masks)} drop_masks for {K} chunks")
        e = self.eng
        self._mark("start")
        if drop_masks is not None:
            masks = [self._check_drop_masks(drop_masks[k], int(chunks[k][0].shape[0])) for k in range(K)]
        elif self.drop_path:
            e.refresh()
            masks = [self.draw_drop_masks(int(chunks[k][0].shape[0])) for k in range(K)]
        else:
            masks = [None] * K
        bank_i, bank_t, starts = self._feature_pass(chunks, masks)
        self._mark("features")
        loss, dfeat = self._bank_head(bank_i, bank_t, starts)
        self._mark("head")
        if not check_features:
            bank_i = bank_t = None
        for k in range(K):
            img, tok = chunks[k]
            pi, pt = self.forward(img, tok, drop_masks=masks[k], _head=False)
            if check_features:
                r0, r1 = starts[k], starts[k + 1]
                for name, now, banked in (("image", pi, bank_i[r0:r1]), ("text", pt, bank_t[r0:r1])):
                    if not torch.equal(now, banked):
                        self._release_saved()
                        raise RuntimeError(f"TrainStep.accumulate(): the {name} features of chunk {k} recomputed in the gradient "
                                           "pass differ from the ones the head was computed from (a kernel on the forward path "
                                           "is not bitwise repeatable)")
            del pi, pt
            g = self.backward(_dfeat=dfeat[k])
            dfeat[k] = None
            acc = self._acc
            if acc is None or acc.shapes != {key: (tuple(t.shape), t.device) for key, t in g.items()}:
                acc = self._acc = _Accumulators(g)
            with torch.cuda.device(e.dev):
                self._mark("backward")
                acc.add(g, 0 if k == 0 else 1)
                self._mark("accumulate")
            del g
        self.last_drop_masks = masks if masks[0] is not None else None
        out = acc.views
        return loss, ({key: t.clone() for key, t in out.items()} if clone else dict(out))

    def _release_saved(self):
        if self.saved is not None:
            self.saved["w"].pop("held", None)
            self.saved = None

    def _feature_pass(self, chunks, masks=None):
        """Pass 1 of accumulate(): -> (bank_i, bank_t bf16 [N, 2E], [first row of every chunk] + [N]).  masks[k]: chunk k's
        stochastic-depth keep masks (None: off)."""
        e = self.eng
        masks = masks if masks is not None else [None] * len(chunks)
        sizes = [int(chunks[k][0].shape[0]) for k in range(len(chunks))]
        starts = [0]
        for b in sizes:
            starts.append(starts[-1] + b)
        N = starts[-1]
        bank_i = torch.empty(N, 2 * e.E, dtype=BF, device=e.dev)
        bank_t = torch.empty(N, 2 * e.E, dtype=BF, device=e.dev)
        for k in range(len(chunks)):
            img, tok = chunks[k]
            pi, pt = self.forward(img, tok, drop_masks=masks[k], _head=False, _update_stats=False)
            self._release_saved()                                                # nothing is kept for a backward
            bank_i[starts[k]:starts[k + 1]] = pi
            bank_t[starts[k]:starts[k + 1]] = pt
        return bank_i, bank_t, starts

    def _bank_head(self, bank_i, bank_t, starts):
        """Pass 2 of accumulate(): -> (loss, [(d image features, d text features, d logit_scale) per chunk])."""
        e = self.eng
        dev, E = e.dev, e.E
        with torch.cuda.device(dev), torch.no_grad():
            N, K = starts[-1], len(starts) - 1
            s_dev = e.model.logit_scale.detach().float().exp()
            a3_i, b3_t = _logit_operands(bank_i, bank_t, E)
            a3_t, b3_i = _logit_operands(bank_t, bank_i, E)
            allI, allT = bank_i[:, :E].contiguous(), bank_t[:, :E].contiguous()

            def blocks(k):                                                       # S_i, S_t [B_k, N]: the N x N matrix never exists
                r0, r1 = starts[k], starts[k + 1]
                return _logits(a3_i[r0:r1], b3_t), _logits(a3_t[r0:r1], b3_i)
            lse = torch.empty(2, N, dtype=F32, device=dev)
            parts = torch.empty(K, dtype=F32, device=dev)
            kept = None
            for k in range(K):
                r0, r1 = starts[k], starts[k + 1]
                S_i, S_t = blocks(k)
                _loss_partial(S_i, S_t, lse[0][r0:r1], lse[1][r0:r1], r0, N, parts[k:k + 1])
                if K == 1:
                    kept = (S_i, S_t)
            loss = parts[0].clone() if K == 1 else parts.sum()
            npad = (N + 63) // 64 * 64
            bt_T, bt_I = hip.transpose_bf16(allT, N, npad), hip.transpose_bf16(allI, N, npad)
            dfeat = []
            for k in range(K):
                r0, r1 = starts[k], starts[k + 1]
                S_i, S_t = kept if kept is not None else blocks(k)               # recomputed: the same bits (deterministic GEMM)
                dfi, dft, dscale = _clip_head_bwd(e, S_i, S_t, allI, allT, lse[:, r0:r1], lse, r0, N, s_dev, bt=(bt_T, bt_I))
                dfeat.append((dfi, dft, dscale.reshape(())))
            return loss, dfeat

    def _mark(self, name):
        """tools/accumulate_bench.py sets self.phase_events = []: a timing event at every phase boundary of accumulate()."""
        if self.phase_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.eng.dev))
            self.phase_events.append((name, ev))

    # ------------------------------------------------------------------ optimizer
    def set_epoch(self, epoch):
        """Apply the yaml's learning-rate schedule (self.schedule, train.from_config) for `epoch` to both parameter groups'
        base rates; the next step() re-points the optimizer table's rates.  No-op without a schedule."""
        sch = self.schedule
        if sch is None:
            return
        if self._base_lr is None:
            self._base_lr = (self.lr, self.lr_share)
        base, base_sh = self._base_lr
        self.lr = sch.lr_at(base, epoch)
        self.lr_share = None if base_sh is None else sch.lr_at(base_sh, epoch)

    def param_groups(self):
        """(name, parameter, lr, weight_decay) for every parameter: module-level param_groups() with this step's settings."""
        return param_groups(self.model, self.lr, self.lr_share, self.wd, self.wd_share, self.without_wd)

    def _packed_destinations(self):
        """{id(parameter): [(first element, element count, packed tensor, scale)]}: the engine's copies of the transformer
        blocks' projection tensors that are plain (scaled) casts of a parameter -- AdamW writes them from the same kernel as
        the parameter itself (msclip_adamw_tensor.pk).  in_proj: the q rows carry head_dim^-0.5 (packing.qkv_weights)."""
        e = self.eng
        out = {}
        for blk in {id(b["w"]): b["w"] for b in list(e.tblk) + [b for b in e.vblk if b is not None]}.values():
            a, mlp = blk.blk.attn, blk.blk.mlp
            d = a.in_proj_weight.shape[1]
            out[id(a.in_proj_weight)] = [(0, d * d, blk.wqkv.view(-1)[:d * d], blk.qscale),
                                         (d * d, 2 * d * d, blk.wqkv.view(-1)[d * d:], 1.0)]
            out[id(a.in_proj_bias)] = [(0, d, blk.bqkv[:d], blk.qscale), (d, 2 * d, blk.bqkv[d:], 1.0)]
            out[id(a.out_proj.weight)] = [(0, blk.wo.numel(), blk.wo.view(-1), 1.0)]
            out[id(mlp.c_fc.weight)] = [(0, blk.wfc.numel(), blk.wfc.view(-1), 1.0)]
            out[id(mlp.c_proj.weight)] = [(0, blk.wpr.numel(), blk.wpr.view(-1), 1.0)]
        return out

    def _adamw_plan(self, grads):
        """The tensor table of the optimizer launch: built once, per step only the gradient addresses are re-pointed;
        rebuilt when the set of gradients changes, the optimizer state is replaced or the engine has re-packed (new copies)."""
        pk_ok = not self.eng.fp8
        sig = (id(self.eng.tblk[0]["w"].wqkv), pk_ok, id(self.state), self.eng.tensor_identity(), self.optimizer, self.always_adapt)
        plan = self._plan
        if plan is not None and plan.sig == sig and len(grads) == plan.ngrads and \
                all(k in grads and grads[k].dtype == F32 and grads[k].numel() == n for k, n in plan.names.items()):
            # same tensors, this step's gradients (fresh allocations on one GPU, the bucket slots at N > 1); the few that
            # arrive as permuted views (depthwise adapter weights) are made contiguous, alive until the launch is queued
            flat = {k: (grads[k] if grads[k].is_contiguous() else grads[k].contiguous()) for k in plan.names}
            plan.hold = flat
            plan.set_grads([flat[k].data_ptr() + 4 * lo for k, lo in plan.pieces])
            if plan.rates_for != (self.lr, self.lr_share, self.wd, self.wd_share):
                groups = {k: (lr, wd) for k, _, lr, wd in self.param_groups()}
                plan.set_rates([groups[k] for k, _ in plan.pieces])
                plan.rates_for = (self.lr, self.lr_share, self.wd, self.wd_share)
            return plan
        if self.nonfinite is not None:                   # a new table counts its skipped runs from 0: keep what the old one counted
            self._skip_base = self._resolve_skips()
            self._skip_seen = 0
        dests = self._packed_destinations() if pk_ok else {}
        items, pieces, names, hold = [], [], {}, []
        for k, p, lr, wd in self.param_groups():
            g = grads.get(k)
            if g is None:
                continue
            g = g.reshape(p.shape).contiguous().view(-1)
            hold.append(g)
            st = self.state.get(k)
            if st is None:
                st = self.state[k] = (torch.zeros_like(p), torch.zeros_like(p))
            pf, mf, vf = p.data.view(-1), st[0].view(-1), st[1].view(-1)
            names[k] = p.numel()
            for lo, n, pk, scale in dests.get(id(p), [(0, p.numel(), None, 1.0)]):
                items.append((pf[lo:lo + n], g[lo:lo + n], mf[lo:lo + n], vf[lo:lo + n], lr, wd, pk, scale))
                pieces.append((k, lo))
        joined = [lo != 0 for _, lo in pieces]                                # the norm's table: one entry per gradient tensor
        if self.optimizer == "lamb":                                          # (and one trust ratio per entry)
            plan = hip.LambPlan(items, joined=joined, always_adapt=self.always_adapt)
        else:
            plan = hip.AdamwPlan(items, joined=joined)
        plan.sig, plan.pieces, plan.names, plan.ngrads = sig, pieces, names, len(grads)
        plan.rates_for = (self.lr, self.lr_share, self.wd, self.wd_share)
        plan.packs = bool(dests)
        plan.hold = hold
        self._plan = plan
        return plan

    # ------------------------------------------------------------------ non-finite guard
    def _resolve_skips(self):
        """-> the number of skipped steps so far.  Waits for the last guarded step()'s copy of the verdict (the one host wait
        of the guard; a no-op where none is pending or it has arrived)."""
        if self._skip_event is not None:
            self._skip_event.synchronize()
            self._skip_event = None
            self._skip_seen = int(self._skip_host[1])
        return self._skip_base + self._skip_seen

    @property
    def skipped_steps(self):
        """step() calls that left the model untouched (host int; reading it waits for the last step()'s verdict).  0 without
        the guard."""
        return self._resolve_skips()

    @property
    def applied_steps(self):
        """step() calls that updated the model: steps - skipped_steps."""
        return self.steps - self._resolve_skips()

    def nonfinite_gradients(self):
        """Names of the parameters whose gradient of the LAST step() held a NaN or an Inf (more precisely: whose chunks of the
        norm's table hold a non-finite partial sum of squares), in the table's order; [] where the step was clean.
        Synchronises (reads the optimizer table's partials); valid until the next step()."""
        plan = self._plan
        if self.nonfinite is None or plan is None or plan.partials is None:
            raise RuntimeError("TrainStep.nonfinite_gradients() needs TrainStep(..., nonfinite=...) and a step() before it")
        return nonfinite_names(plan.partials[:plan.n_partials].cpu(), list(plan.names.items()))

    @hip.off_default_stream
    def step(self, grads, world_average=False):
        """AdamW on the module's fp32 parameters (msclip_adamw_multi), which also writes the engine's bf16 copies of the
        transformer blocks' projections; the engine re-packs the rest (conv side, heads).  backward() already returns
        rank-averaged gradients; world_average=True averages here instead, tensor by tensor (for gradients produced with
        backward(reduce=False)).

        With self.clip_grad_norm set (not None / 0): the step of torch.nn.utils.clip_grad_norm_(parameters, clip_grad_norm,
        norm_type=2, error_if_nonfinite=False) followed by AdamW, all on the device: the L2 norm
        over every gradient of the dict (one entry per Parameter object, logit_scale included), coef = min(1, max_norm /
        (norm + 1e-6)), and the optimizer sees g * coef.  Unlike torch, nothing is written back: the gradient dict is left
        as produced.  With ema_decay set, one msclip_ema_multi call follows the optimizer's on the same stream (once per step(),
        whatever number of chunks accumulate() summed; every rank updates its own shadow from parameters that are identical
        across ranks: no collective) and self.ema_updates counts it.  Afterwards self.last_grad_norm / self.last_clip_coef are 0-dim device tensors, views of the optimizer
        table's block that are valid until the next step(); .item() on them is the caller's choice of when to synchronise
        (step() never does).  Without the non-finite guard (below) a non-finite norm is not skipped: it reaches the parameters
        as it does in torch.
        Ranks: the norm is taken after the rank averaging (backward()'s, or world_average=True's), so it is the norm of the
        averaged gradient, identical on every rank, with no further collective.  After accumulate() it is the norm of the SUM
        over the chunks, which is what a one-shot step on the whole batch clips.

        optimizer = "lamb": three calls in place of the AdamW launch (msclip_lamb_partials -> msclip_lamb_ratios ->
        msclip_lamb_apply, include/msclip_ext3.h), behind the two of the clip norm when clip_grad_norm is set and in front of
        the EMA's: for every Parameter object u = m_hat / (sqrt(v_hat) + eps) + wd * w from the new moments, r = ||w|| / ||u||
        (1 where either norm is 0 or NaN; min(r, 1) with trust_clip), w -= lr * r * u where wd != 0 or always_adapt, w -= lr * u
        elsewhere.  The norms are over the whole Parameter (in_proj_weight, two entries of the table, has one ratio) and, like
        the clip norm, come from parameters and averaged gradients that are identical on every rank: no collective.
        Afterwards self.last_trust_ratio / last_param_norm / last_update_norm are {parameter name: 0-dim device view}, valid
        until the next step() and never read back here; last_trust_ratio holds r as computed, also for a tensor whose step
        did not use it.  They are None under adamw.

        nonfinite = "skip" / "raise" (include/msclip_ext4.h): the norm's two calls run always (msclip_grad_sumsq ->
        msclip_clip_coef_guarded; last_grad_norm is set also without clipping, last_clip_coef stays None then) and leave a
        verdict on the device; the update is msclip_adamw_multi_guarded / msclip_lamb_apply_guarded, which writes nothing where
        any partial is NaN or Inf: parameters, moments and packed copies keep their bits.  The trust ratios of a skipped
        step mean nothing; the EMA shadows take one more pull toward the unchanged parameters (what timm's loop does when a
        GradScaler skips).  Forward-side state (BatchNorm running statistics under bn="batch", the stochastic-depth generator)
        is not undone.  The step number handed to the library -- the bias corrections' exponent -- is the count of APPLIED
        updates: after its launches step() queues a non-blocking copy of {verdict, skipped total} into pinned host memory and
        records an event, without waiting; the NEXT step() waits for that event, i.e. for the previous step's optimizer phase,
        and passes steps - skipped.  So with the guard on the host runs at most one step ahead of the device, and this is the
        only case in which step() waits; self.steps keeps counting calls.  self.last_skipped is the verdict as a 0-dim device
        int view (valid until the next step()), skipped_steps / applied_steps are host ints, nonfinite_gradients() names
        the tensors.  "raise" reads this step's verdict (a synchronisation) and raises FloatingPointError after everything else
        step() does.  Ranks: the verdict is taken on the averaged gradient, so it is identical on every rank with no collective
        (not run on more than one rank).  After accumulate() it is the verdict on the sum over the chunks.  A run without
        skips is bitwise the unguarded run."""
        if self.lr is None:
            raise ValueError("TrainStep.step() needs a learning rate: TrainStep(model, lr=...) or train.from_config(model, config)")
        self._ema_live("step")
        if hasattr(grads, "check_fresh"):
            grads.check_fresh()
        guard = self.nonfinite is not None
        skipped = self._resolve_skips() if guard else 0      # (before the count moves: the previous step's verdict is in)
        self.steps += 1
        max_norm = float(self.clip_grad_norm) if self.clip_grad_norm else None
        with torch.no_grad():
            if world_average:
                world_average_(grads)
            plan = self._adamw_plan(grads)
            if guard:
                plan.run(self.betas[0], self.betas[1], self.eps, self.steps - skipped, max_norm, guard=True, **self._run_options)
            else:
                plan.run(self.betas[0], self.betas[1], self.eps, self.steps, max_norm, **self._run_options)
            plan.hold = None
            if self._ema is not None:                # behind the AdamW launch on the same stream: the shadows follow the new values
                self._ema.plan.run(self.ema_decay)
                self.ema_updates += 1
            if guard and plan.n:                     # {verdict, skipped total of this table} -> pinned memory, read by the next step()
                if self._skip_host is None:
                    self._skip_host = torch.zeros(2, dtype=torch.int32).pin_memory()
                self._skip_host.copy_(plan.guard_state[:2], non_blocking=True)
                self._skip_event = torch.cuda.Event()
                self._skip_event.record()
                self.last_skipped = plan.skip
        if max_norm is None:
            self.last_grad_norm, self.last_clip_coef = (plan.norm if guard else None), None
        else:
            self.last_grad_norm, self.last_clip_coef = plan.norm, plan.coef
        if self.optimizer == "lamb":
            order = list(dict.fromkeys(k for k, _ in plan.pieces))             # the table's parameters, in its order
            self.last_trust_ratio, self.last_param_norm, self.last_update_norm = (
                {k: row[i] for i, k in enumerate(order)} for row in (plan.ratio, plan.param_norm, plan.update_norm))
        if plan.packs:
            self.eng.repack_after_optimizer()
        else:
            self.eng.refresh(force=True)
        if self.nonfinite == "raise" and plan.n and int(plan.skip.item()):
            names = self.nonfinite_gradients()
            raise FloatingPointError(f"TrainStep.step(): step {self.steps} was skipped, NaN or Inf in the gradient of {names} "
                                     f"({len(names)} of {len(plan.names)} tensors); parameters and optimizer state are untouched")

    # ------------------------------------------------------------------ weight EMA
    def _ema_live(self, what):
        if self._ema_assigned:
            raise RuntimeError(f"TrainStep.{what}() between ema_assign() and ema_resume(): the model holds the shadow weights "
                               "(evaluate or save, then call ema_resume())")

    @hip.off_default_stream
    def ema_assign(self):
        """Put the shadow weights into the model (evaluation, saving): every parameter and its shadow exchange their VALUES in
        place -- the parameters' addresses are in the optimizer's and the engine's tables, so no storage changes hands --
        and the engine re-packs.  Until ema_resume() the shadow arena holds the live weights, and step() / forward() /
        accumulate() / a second ema_assign() raise RuntimeError.  The names follow the reference's unreleased EMA class
        (lib/utils/utils.py:188-192: shadow, assign, resume)."""
        if self._ema is None:
            raise RuntimeError("TrainStep.ema_assign() needs TrainStep(..., ema_decay=...)")
        self._ema_live("ema_assign")
        self._ema_conv_pack = self.eng.conv_pack
        self._ema.swap()
        self._ema_assigned = True
        self.eng.refresh(force=True)

    @hip.off_default_stream
    def ema_resume(self):
        """Undo ema_assign(): the live weights return to the model bit for bit, the shadows to the arena; the engine re-packs,
        and where the conv side's operands had last been written by an optimizer step's table-driven re-pack
        (Engine.repack_after_optimizer: equal to the full pack's to an fp32 ulp, not bitwise) that re-pack runs again, so the
        engine serves the bits it served before ema_assign()."""
        if not self._ema_assigned:
            raise RuntimeError("TrainStep.ema_resume() without an ema_assign() before it")
        self._ema.swap()
        self._ema_assigned = False
        self.eng.refresh(force=True)
        if self._ema_conv_pack == "table":
            self.eng.repack_after_optimizer()

    def ema_weights(self):
        """Context manager: ema_assign() on entry, ema_resume() on exit (also when the body raises)."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.ema_assign()
            try:
                yield self
            finally:
                self.ema_resume()
        return scope()


def _logit_operands(a, ball, E):
    """The K = 3E operand pair of the logits A_loc @ B_all^T from two gather payloads [rows, 2E] (bf16 hi | lo parts of the
    fp32 features): [hi | hi | lo] of a, [hi | lo | hi] of ball -- hi.hi + hi.lo + lo.hi in one GEMM."""
    return (torch.cat([a[:, :E], a[:, :E], a[:, E:]], dim=1), torch.cat([ball[:, :E], ball[:, E:], ball[:, :E]], dim=1))


def _logits(a3, b3):
    """-> S = a3 @ b3^T, fp32 [rows of a3, rows of b3]."""
    S = torch.empty(a3.shape[0], b3.shape[0], dtype=F32, device=a3.device)
    hip.gemm(a3, b3, S)
    return S


def _loss_partial(S_i, S_t, lse_i, lse_t, off, n, out):
    """Row blocks S_i / S_t [R, n] (labels off .. off + R) -> their log-sum-exps into lse_i / lse_t [R] and their share of the
    symmetric cross-entropy over n pairs into out [1]."""
    hip.lse_rows(S_i, lse_i)
    hip.lse_rows(S_t, lse_t)
    hip.clip_loss_partial(lse_i, lse_t, S_i, off, 1.0 / (2.0 * n), out)


def _clip_head_bwd(e, S_i, S_t, allI, allT, lse_loc, lse_all, off, n, scale, bt=None):
    """Backward of the contrastive head for the row blocks S_i / S_t [R, n] (this rank's -- or, in accumulate(), this chunk's --
    image rows and caption rows, labels off .. off + R): -> (d image features, d text features [R, E] fp32, [1] sum G S =
    d loss / d logit_scale of these rows).  allI (carries the scale) / allT: the hi parts of all n rows; bt: their transposes
    (allT^T, allI^T) [E, npad] when the caller already holds them."""
    dev, E = e.dev, e.E
    npad = (n + 63) // 64 * 64
    wgt = 1.0 / (2.0 * n)

    def side(S, b_all, b_t, lse_row, lse_col, want_dscale):
        G = torch.empty(S.shape[0], npad, dtype=BF, device=dev)
        dsp = torch.empty(S.shape[0], dtype=F32, device=dev) if want_dscale else None
        hip.clip_loss_bwd_g(S, lse_row, lse_col, off, wgt, G, dsp)
        if b_t is None:
            b_t = hip.transpose_bf16(b_all, n, npad)                                       # [E, npad]
        d = torch.empty(S.shape[0], E, dtype=F32, device=dev)
        hip.gemm(G, b_t, d)                                                                # dA = G @ B_all (scale: below)
        return d, dsp
    dfi, dsp = side(S_i, allT, bt[0] if bt else None, lse_loc[0], lse_all[1], True)
    dfi *= scale                                                                            # d(image features) = scale * G_i @ T_all
    dft, _ = side(S_t, allI, bt[1] if bt else None, lse_loc[1], lse_all[0], False)         # allI already carries the scale
    return dfi, dft, hip.colsum(dsp.view(-1, 1))                                            # sum_r sum_j G S


def _rs_rows(rs, k, r0, r1, first_row_of_text):
    """A launch over rows [r0, r1): its slice of branch k's row scales (text-only launches, or no stochastic depth: none)."""
    return rs[k][r0:r1] if (rs is not None and r0 < first_row_of_text) else None


def _split_hi_lo(f):
    """---- loss.  The inference path forms its logits from bf16 unit features (error ~0.03 on a logit at T = 1/0.07:
    fine for a loss value, but it perturbs every softmax probability by a few percent and with it the whole
    gradient).  The training step splits each fp32 feature into bf16 hi + lo parts and contracts
    [hi | hi | lo] . [hi | lo | hi] in one K = 3E GEMM: logits to ~2^-16 relative, still on the bf16 MFMA path."""
    hi = hip.cast_bf16(f)
    lo = hip.cast_bf16(f - hi.float())
    return torch.cat([hi, lo], dim=1)                                              # [B, 2E]: the gather payload


def _unscale_q(g):                                                                 # packed q rows = 64^-0.5 * W_q
    g[:g.shape[0] // 3] *= 0.125
    return g


class _Grads(dict):
    """{key: gradient} of one backward(); with a comm.GradReducer every gradient enters its all-reduce bucket as it is set."""

    def __init__(self, reducer, dev):
        dict.__init__(self)
        self.reducer, self.dev = reducer, dev

    def __setitem__(self, k, v):
        dict.__setitem__(self, k, v)
        if self.reducer is not None:
            self.reducer.add(k, v)

    def slot(self, k, shape):
        """Where gradient k should be written if it can be born inside its all-reduce bucket (else None)."""
        return self.reducer.reserve(k, shape, self.dev) if self.reducer is not None else None


class _BackwardPass:
    """What the phases of ONE TrainStep.backward() share: the gradients, the deferred column sums, the queue of wide weight
    gradients, the W^T operands, dX (the gradient of the token matrix, [M, D] fp32) and dXC (of the last block's live rows),
    the conv side's object.  TrainStep.backward() is the driver that calls the phases in order."""

    def __init__(self, ts, sv, reducer):
        self.ts, self.e, self.sv = ts, ts.eng, sv
        self.dev, self.D = self.e.dev, self.e.D
        self.Bi, self.Bt, self.Mv, self.M = sv["Bi"], sv["Bt"], sv["Mv"], sv["M"]
        self.grads = _Grads(reducer, self.dev)
        # Column sums nothing on the critical path reads (LayerNorm parameter gradients, bias gradients): their producers leave
        # per-block partial matrices, ONE msclip_colsum_multi launch folds all of them behind the transformer's backward (round 5:
        # ~120 msclip_colsum launches per step, 1.1 ms of the main queue)
        self.folds = hip.FoldPlan(self.dev)
        # the four wide weight gradients of a block: operand transposes on the lane at once, the split-K GEMM of job k
        # on THIS stream when job k + 1 is created (its transposes have run under the kernels issued in between)
        self.pending = []
        self.wts, self.wt_ready = {}, {}
        self.dX = self.dXC = self.conv = None

    def block_key(self, i, b):
        """state_dict prefix of tower entry b's block i."""
        return f"visual.transformer.resblocks.{i}" if b is self.e.vblk[i] else f"transformer.resblocks.{i}"

    def names(self, i):
        """{id(block weights): their prefix} of layer i (one Parameter set under its visual.* name where the towers share it)."""
        return {id(b["w"]): self.block_key(i, b) for b in (self.e.tblk[i], self.e.vblk[i]) if b is not None}

    def fold_into(self, part, then, scale_n=0, scale=1.0):
        self.folds.add(part, then, scale_n=scale_n, scale=scale)

    def ln_param_grads(self, part, key):
        """part: (dgamma | dbeta) partials [blocks, 2 C] of a LayerNorm backward -> grads[key.weight], grads[key.bias]."""
        grads = self.grads

        def then(r):
            c = r.shape[0] // 2
            grads[key + ".weight"], grads[key + ".bias"] = r[:c], r[c:]
        self.fold_into(part, then)

    def set_bias(self, key, val):
        """val: the bias gradient itself, or a 2-D matrix of partial sums still to be folded."""
        grads = self.grads                                   # (the deferred lambda holds the gradients, not this object)
        if val.dim() == 2:
            self.fold_into(val, lambda r: grads.__setitem__(key, r))
        else:
            grads[key] = val

    def flush_wgrads(self):
        pending, grads = self.pending, self.grads
        while pending:
            k, job, shape = pending.pop(0)
            grads[k] = job.finish(grads.slot(k, shape))

    def wide_wgrad(self, k, dy, x, rows, shape, post=None):
        self.flush_wgrads()
        self.pending.append((k, gradgemm.WgradJob(dy, x, rows, post=post), shape))

    def heads(self, _dfeat):
        """The contrastive head (or accumulate()'s feature gradients), dX / dXC, the conv side's object, both towers' heads."""
        ts, e, sv, grads, dev, Bi = self.ts, self.e, self.sv, self.grads, self.dev, self.Bi
        # ---- contrastive head: dL/dS blocks of this rank's image rows and caption rows
        if _dfeat is not None:
            dfi, dft, dls = _dfeat
            grads["logit_scale"] = dls
        else:
            dfi, dft, dscale = _clip_head_bwd(e, sv["S_i"], sv["S_t"], sv["allI"], sv["allT"], sv["lse_loc"], sv["lse_all"],
                                              sv["off"], sv["n"], sv["scale"])
            if sv["coll"]:
                dist.all_reduce(dscale)
            # S already carries the scale: dL/dscale = sum G S / scale; logit_scale = log(scale) => dL/dlogit_scale = sum G S
            grads["logit_scale"] = dscale.reshape(())
        self.dX = torch.zeros(self.M, self.D, dtype=F32, device=dev)
        if e.patch:
            self.conv = None                         # patch-conv stem: its weight gradient at the end (_patch_wgrad)
        elif ts.bn == "batch":
            self.conv = ts.convbn                    # holds the raw conv outputs / batch statistics of this forward
        else:
            self.conv = ConvSideBackward(ts)
            self.conv.begin(sv["img"], sv["w"], Bi)
        compact_x = sv.get("compact")                 # [Bi + Bt, D]: the last block ran its row-wise tail on the live rows only
        self.dXC = torch.zeros(Bi + self.Bt, self.D, dtype=F32, device=dev) if compact_x is not None else None
        if compact_x is not None:
            self.head(sv["fv_raw"], dfi, sv["hv"], e.w_vproj, e.ln_post, "visual.proj", "visual.ln_post", c0=0)
            self.head(sv["ft_raw"], dft, sv["ht"], e.w_tproj, e.ln_final, "text_projection", "ln_final", c0=Bi)
        else:
            self.head(sv["fv_raw"], dfi, sv["hv"], e.w_vproj, e.ln_post, "visual.proj", "visual.ln_post", row_mul=e.Lv)
            self.head(sv["ft_raw"], dft, sv["ht"], e.w_tproj, e.ln_final, "text_projection", "ln_final", row_idx=sv["eot"])

    def head(self, feat_raw, dfeat, hrow, w_proj, ln, key_proj, key_ln, row_idx=None, row_mul=1, c0=None):
        sv = self.sv
        dfr = torch.empty_like(feat_raw)
        hip.l2norm_bwd(feat_raw, dfeat, dfr)
        dfr_b = hip.cast_bf16(dfr)
        self.grads[key_proj] = _wgrad(hrow, dfr_b, hrow.shape[0])                      # [D, E] like the parameter
        dh = torch.empty(hrow.shape[0], self.D, dtype=F32, device=self.dev)            # fp32: it feeds column sums
        hip.gemm(dfr_b, w_proj.t().contiguous(), dh)                                   # dfr [B, E] @ W [E, D]
        if c0 is not None:                        # compact rows c0 .. of x_out / dXC, one per sample
            n_ = hrow.shape[0]
            part, _ = hip.layernorm_bwd(sv["x_out"][c0:c0 + n_], dh, ln.g, self.dXC[c0:c0 + n_], n_, fold=False)
        else:
            part, _ = hip.layernorm_bwd(sv["x_out"], dh, ln.g, self.dX, hrow.shape[0], row_idx=row_idx, row_mul=row_mul, fold=False)
        self.ln_param_grads(part, key_ln)

    def cast_with_bias_sums(self, dX, dY, r_lo, groups, rs=None):
        """dY[r_lo:M] = bf16(dX[r_lo:M]) -- the operand of a projection's dgrad / wgrad GEMMs -- and {id(block
        weights): column sums of the group's rows} = that projection's bias gradient; one pass over dX when a
        single (shared) weight set covers all rows.  rs (fp32 [M], stochastic depth): copy and sums of rs[row] * dX[row]
        -- what everything upstream of the projection's scaled residual add sees -- from the same one pass per group."""
        M = self.M
        if rs is not None:
            return {id(bw): hip.cast_bf16_colsum(dX[r0:r1], dY[r0:r1], fold=False, row_scale=rs[r0:r1])[1] for r0, r1, bw in groups}
        if len(groups) == 1 and groups[0][0] == r_lo and groups[0][1] == M:
            _, s = hip.cast_bf16_colsum(dX[r_lo:M], dY[r_lo:M], fold=False)    # partial sums: folded with the others (set_bias)
            return {id(groups[0][2]): s}
        hip.cast_bf16(dX[r_lo:M], dY[r_lo:M])
        return {id(bw): hip.colsum(dX[r0:r1]) for r0, r1, bw in groups}

    def transposed_weights(self):
        """---- the dgrad GEMMs' W operands: W^T of every projection (bf16 [K, N]; the weights changed in the last optimizer
        step), all of them up front on the lane stream with this library's transpose kernel, last block first, one event
        per block -- not four ATen transposed copies per block on the main queue (74 launches, 1.8 ms per step)"""
        ts, e, wts, wt_ready = self.ts, self.e, self.wts, self.wt_ready
        if not gradgemm.lane_enabled():
            return
        sets = []
        for i in reversed(range(e.n_layers)):
            for blk in (e.tblk[i], e.vblk[i]):
                if blk is not None and all(blk["w"] is not b for b in sets):
                    sets.append(blk["w"])
        srcs = [t for bw in sets for t in (bw.wpr, bw.wfc, bw.wo, bw.wqkv)]
        ln_s = gradgemm.lane(self.dev)
        with hip.forked(ln_s) as cur_s:
            if all(t.shape[0] % 64 == 0 for t in srcs):
                # ONE table-driven launch for all of them (48 launches one by one kept the host busy for 0.6 ms at the start
                # of the backward, the main queue idle behind it); the table lives while the packed weights do not move
                plan = ts._wt_plan
                if plan is None or plan.key != tuple(t.data_ptr() for t in srcs):
                    plan = ts._wt_plan = hip.TransposePlan(srcs)
                outs = plan.run()
                done = torch.cuda.Event()
                done.record(ln_s)
                for j, bw in enumerate(sets):
                    wts[id(bw)] = tuple(outs[4 * j:4 * j + 4])
                    wt_ready[id(bw)] = done              # (one launch, one event: whichever weight set is asked for first waits for it)
            else:
                for bw in sets:
                    wts[id(bw)] = tuple(hip.transpose_bf16(t, t.shape[0], t.shape[0]) for t in (bw.wpr, bw.wfc, bw.wo, bw.wqkv))
                    for t in wts[id(bw)]:
                        t.record_stream(cur_s)
                    wt_ready[id(bw)] = torch.cuda.Event()
                    wt_ready[id(bw)].record(ln_s)

    def w_t(self, bw, which):
        """W^T of block weights bw: 0 c_proj [4D, D]^T.., 1 c_fc, 2 out_proj, 3 in_proj (packed: q rows scaled)."""
        if id(bw) in self.wts:
            ev = self.wt_ready.pop(id(bw), None)
            if ev is not None:
                torch.cuda.current_stream(self.dev).wait_event(ev)
            return self.wts[id(bw)][which]
        return (bw.wpr, bw.wfc, bw.wo, bw.wqkv)[which].t().contiguous()

    def ln_bwd_segments(self, x_saved, dlno, segs, groups, r_lo, which, i, dY_next, rs=None):
        """LayerNorm backward (`which` = "ln1" / "ln2" of block i) of every row segment: dX += its input gradient.  With
        dY_next (bf16 [M, D]) the same pass leaves bf16(new dX) there -- the output gradient of the projection in front of
        this LayerNorm point, operand of its dgrad / wgrad GEMMs -- and returns {id(block weights): that projection's bias
        gradient} from per-block column sums (no cast_bf16_colsum pass over dX); else returns None.  rs (fp32 [M], with
        dY_next): that projection sits behind a DropPath -- the copy and the sums of the image rows carry rs[row], dX does not."""
        dX, D, dev, Mv = self.dX, self.D, self.dev, self.Mv
        parts = {}
        for r0, r1, b in segs:
            kw = {}
            if dY_next is not None:
                gid = next(id(bw) for g0, g1, bw in groups if g0 <= r0 and r1 <= g1)
                first = gid not in parts
                if first:
                    parts[gid] = torch.empty(hip.LN_PART_BLOCKS, D, dtype=F32, device=dev)
                kw = dict(dxb=dY_next[r0:r1], sum_part=parts[gid], sum_accumulate=not first,
                          row_scale=rs[r0:r1] if (rs is not None and r0 < Mv) else None)
            part, _ = hip.layernorm_bwd(x_saved[r0 - r_lo:r1 - r_lo], dlno[r0:r1], b[which].g, dX[r0:r1], r1 - r0, fold=False, **kw)
            self.ln_param_grads(part, f"{self.block_key(i, b)}.{'ln_1' if which == 'ln1' else 'ln_2'}")
        return parts if dY_next is not None else None          # (partial sums: set_bias folds them)

    def cast_c(self, cm, k):
        """bf16(dXC) and, per weight group, its column sums -- of rs_c[k][row] * dXC[row] behind a DropPath: one
        library pass per group writes the scaled copy and the scaled fp32 rows (a partial row per row), which
        the unscaled path's own colsum launch then folds (same shape, same order: scale 1 gives its bits)."""
        dXC, rs_c = self.dXC, cm["rs"]               # rs_c: [2, nc] row scales of the live rows (stochastic depth), or None
        if rs_c is None:
            return hip.cast_bf16(dXC), {id(bw): hip.colsum(dXC[r0:r1]) for r0, r1, bw in cm["cgroups"]}
        y = torch.empty(dXC.shape[0], self.D, dtype=BF, device=self.dev)
        return y, {id(bw): hip.cast_bf16_colsum(dXC[r0:r1], y[r0:r1], row_scale=rs_c[k, r0:r1], blocks=r1 - r0)[1]
                   for r0, r1, bw in cm["cgroups"]}

    def compact_tail(self, i, L):
        """The last block's row-wise tail ran on the Bi + Bt live rows (TrainStep._block_forward): its backward on the same rows.
        dXC holds the heads' gradient wrt the block's output at those rows; every other row's is zero.
        -> (dlno, dao, dqkv) for the attention backward and in_proj."""
        e, grads, dX, dXC, D, dev, Bi, M = self.e, self.grads, self.dX, self.dXC, self.D, self.dev, self.Bi, self.M
        w_t, names, cm = self.w_t, self.names(i), L["compact"]
        nc = Bi + self.Bt
        xm_c, lno2_c, h_c, hid_c, ao_c = cm["x_mid"], cm["lno2"], cm["h"], cm["hid"], cm["ao"]
        dlno2_c = torch.empty(nc, D, dtype=F32, device=dev)
        dy_c, bsum_c = self.cast_c(cm, 1)
        for r0, r1, bw in cm["cgroups"]:
            p = names[id(bw)]
            grads[p + ".mlp.c_proj.weight"] = _wgrad(dy_c[r0:r1], hid_c[r0:r1], r1 - r0)
            grads[p + ".mlp.c_proj.bias"] = bsum_c[id(bw)]
            dh_c = torch.empty(r1 - r0, 4 * D, dtype=BF, device=dev)
            hip.quickgelu_bwd(h_c[r0:r1], _dgrad(dy_c[r0:r1], w_t(bw, 0)), dh_c)
            grads[p + ".mlp.c_fc.weight"] = _wgrad(dh_c, lno2_c[r0:r1], r1 - r0)
            grads[p + ".mlp.c_fc.bias"] = hip.colsum(dh_c)
            _dgrad(dh_c, w_t(bw, 1), dlno2_c[r0:r1])
        for (c0, c1), b in (((0, Bi), e.vblk[i]), ((Bi, nc), e.tblk[i])):
            part, _ = hip.layernorm_bwd(xm_c[c0:c1], dlno2_c[c0:c1], b["ln2"].g, dXC[c0:c1], c1 - c0, fold=False)
            self.ln_param_grads(part, self.block_key(i, b) + ".ln_2")
        # dXC is now the gradient wrt the rows behind the attention (x_mid): out_proj on the compact rows, then both
        # results go back to their rows of the token matrix -- the attention output's gradient (zero elsewhere) and,
        # through the residual connection, the block input's
        dy2_c, bsum_c = self.cast_c(cm, 0)
        dao_c = torch.empty(nc, D, dtype=BF, device=dev)
        for r0, r1, bw in cm["cgroups"]:
            p = names[id(bw)]
            grads[p + ".attn.out_proj.weight"] = _wgrad(dy2_c[r0:r1], ao_c[r0:r1], r1 - r0)
            grads[p + ".attn.out_proj.bias"] = bsum_c[id(bw)]
            _dgrad(dy2_c[r0:r1], w_t(bw, 2), dao_c[r0:r1])
        rows_c = cm["crow"].long()
        dao = torch.zeros(M, D, dtype=BF, device=dev)
        dao.index_copy_(0, rows_c, dao_c)
        dX.index_copy_(0, rows_c, dXC)                   # (dX is still all zero here: nothing but the heads wrote a gradient yet)
        dlno = torch.empty(M, D, dtype=F32, device=dev)
        dqkv = torch.empty(M, 3 * D, dtype=BF, device=dev)
        return dlno, dao, dqkv

    def mlp(self, i, L, carry):
        """MLP half of block i over all rows -> dlno, ln_2's output gradient.  carry: (dY, bias sums) or None (cast here)."""
        dX, D, dev, M, w_t, names = self.dX, self.D, self.dev, self.M, self.w_t, self.names(i)
        r_lo, groups = L["r_lo"], L["groups"]
        hid = L["hid"]
        if carry is not None:
            dY, bsum = carry
        else:
            dY = torch.empty(M, D, dtype=BF, device=dev)
            bsum = self.cast_with_bias_sums(dX, dY, r_lo, groups, rs=L["rs"][1] if L["rs"] is not None else None)
        # gradients of the LayerNorm outputs stay fp32: they are only read by the LayerNorm backward, whose dbeta /
        # dgamma are column sums of nearly cancelling terms (a bf16 dy costs 10-30 % on those sums at small batch)
        dlno = torch.empty(M, D, dtype=F32, device=dev)
        for r0, r1, bw in groups:
            p = names[id(bw)]
            self.wide_wgrad(p + ".mlp.c_proj.weight", dY[r0:r1], hid[r0:r1], r1 - r0, (D, 4 * D))
            self.set_bias(p + ".mlp.c_proj.bias", bsum[id(bw)])
        dh = torch.empty(M, 4 * D, dtype=BF, device=dev)
        dh_part = {}
        for r0, r1, bw in groups:
            if (r1 - r0) % 256 == 0:
                # dh = (dY . W_proj) * QuickGELU'(h): the activation's derivative in the dgrad GEMM's epilogue, which
                # also leaves dh's column sums per 128 rows (c_fc's bias gradient without a second pass over dh)
                dh_part[id(bw)] = torch.empty((r1 - r0) // 128, 4 * D, dtype=F32, device=dev)
                hip.gemm(dY[r0:r1], w_t(bw, 0), dh[r0:r1], resid=L["h"][r0:r1], resid_kind=hip.RESID_GELUGRAD,
                         colsum_part=dh_part.get(id(bw)))
            else:
                dhid = _dgrad(dY[r0:r1], w_t(bw, 0))
                hip.quickgelu_bwd(L["h"][r0:r1], dhid, dh[r0:r1])
        del hid
        for r0, r1, bw in groups:
            p = names[id(bw)]
            self.wide_wgrad(p + ".mlp.c_fc.weight", dh[r0:r1], L["lno2"][r0:r1], r1 - r0, (4 * D, D))
            if id(bw) in dh_part:
                self.set_bias(p + ".mlp.c_fc.bias", dh_part[id(bw)])
            else:
                self.grads[p + ".mlp.c_fc.bias"] = gradgemm.on_lane(lambda a=dh[r0:r1]: hip.colsum(a), dh)
            _dgrad(dh[r0:r1], w_t(bw, 1), dlno[r0:r1])
        del dh
        return dlno

    def out_proj(self, i, L, dlno):
        """attention half.  dX behind the ln_2 backward is out_proj's output gradient: its bf16 copy and bias sums leave with that pass
        -> (dao, dqkv): the attention output's gradient and the matrix the attention backward writes."""
        D, dev, M, names = self.D, self.dev, self.M, self.names(i)
        r_lo, segs, groups = L["r_lo"], L["segs"], L["groups"]
        dY2 = torch.empty(M, D, dtype=BF, device=dev)          # not dY again: the lane stream may still read it (c_proj wgrad)
        rs_a = L["rs"][0] if L["rs"] is not None else None
        bsum = self.ln_bwd_segments(L["x_mid"], dlno, segs, groups, r_lo, "ln2", i, dY2, rs=rs_a)
        dao = torch.empty(M, D, dtype=BF, device=dev)
        dqkv = torch.empty(M, 3 * D, dtype=BF, device=dev)      # attention_bwd writes every row of the towers that ran
        for r0, r1, bw in groups:
            p = names[id(bw)]
            self.wide_wgrad(p + ".attn.out_proj.weight", dY2[r0:r1], L["ao"][r0:r1], r1 - r0, (D, D))
            self.set_bias(p + ".attn.out_proj.bias", bsum[id(bw)])
            _dgrad(dY2[r0:r1], self.w_t(bw, 2), dao[r0:r1])
        return dao, dqkv

    def attention(self, i, L, dao, dqkv):
        """the attention backward also leaves every sample's token sums of its dqkv rows (in_proj's bias gradient = their
        sum over the samples: 1 024 x 3 D fp32 to fold instead of a second pass over dqkv [M, 3 D]); the query-blocked
        form of the long sequences does not carry them -> those sums (qpart, [Bi + Bt, 3 D]) or None."""
        e, sv, Bi, Bt, Mv, M = self.e, self.sv, self.Bi, self.Bt, self.Mv, self.M
        qpart = None
        if e.Lv <= 96 and (sv["cap"] is not None or e.Lt <= 96):
            qpart = torch.empty(Bi + Bt, 3 * self.D, dtype=F32, device=self.dev)
        if e.vblk[i] is not None:
            hip.attention_bwd(L["qkv"][:Mv], L["ao"][:Mv], dao[:Mv], dqkv[:Mv], Bi, e.Lv, e.heads, False,
                              colsum_part=qpart[:Bi] if qpart is not None else None)
        if sv["cap"] is not None:
            hip.attention_bwd_varlen(L["qkv"][Mv:M], L["ao"][Mv:M], dao[Mv:M], dqkv[Mv:M], sv["cap"].cu, Bt, sv["Lmax"],
                                     e.heads, True, pad_rows=sv["pad"], colsum_part=qpart[Bi:] if qpart is not None else None)
        else:
            hip.attention_bwd(L["qkv"][Mv:M], L["ao"][Mv:M], dao[Mv:M], dqkv[Mv:M], Bt, e.Lt, e.heads, True,
                              colsum_part=qpart[Bi:] if qpart is not None else None)
        return qpart

    def in_proj(self, i, L, dqkv, dlno, qpart):
        """in_proj of block i: weight gradient, bias gradient (from qpart, or dqkv's column sums on the lane), dlno <- ln_1's."""
        grads, D, Bi, Bt, Mv, names = self.grads, self.D, self.Bi, self.Bt, self.Mv, self.names(i)
        for r0, r1, bw in L["groups"]:
            p = names[id(bw)]
            self.wide_wgrad(p + ".attn.in_proj_weight", dqkv[r0:r1], L["lno1"][r0:r1], r1 - r0, (3 * D, D),
                            post=_unscale_q)                                        # wrt the PACKED weight, scaled back
            if qpart is not None:
                self.fold_into(qpart[(0 if r0 < Mv else Bi):(Bi + Bt if r1 > Mv else Bi)],
                               lambda r, k=p + ".attn.in_proj_bias": grads.__setitem__(k, r), scale_n=D, scale=0.125)
            else:
                grads[p + ".attn.in_proj_bias"] = gradgemm.on_lane(lambda a=dqkv[r0:r1]: _unscale_q(hip.colsum(a)), dqkv)
            _dgrad(dqkv[r0:r1], self.w_t(bw, 3), dlno[r0:r1])

    def ln1_and_carry(self, i, L, dlno):
        """dX behind the ln_1 backward is the output gradient of the block below's c_proj -- unless a lateral adapter's token
        path adds to the image rows first, or the block below runs other rows -> the block below's carry, (dY, bias sums), or None."""
        r_lo, segs, groups = L["r_lo"], L["segs"], L["groups"]
        below = self.sv["layers"][i - 1] if i > 0 else None
        same = (below is not None and L["adapter"] is None and below["r_lo"] == r_lo and
                [(a, b_) for a, b_, _ in below["segs"]] == [(a, b_) for a, b_, _ in segs] and
                [(a, b_) for a, b_, _ in below["groups"]] == [(a, b_) for a, b_, _ in groups])
        dY_below = torch.empty(self.M, self.D, dtype=BF, device=self.dev) if same else None
        # (behind a DropPath of the block below: its MLP branch's scale rides on this pass)
        bs = self.ln_bwd_segments(L["x_in"], dlno, segs, groups, r_lo, "ln1", i, dY_below,
                                  rs=below["rs"][1] if (dY_below is not None and below["rs"] is not None) else None)
        if bs is None:
            return None
        # keyed by THIS block's weight sets; the block below holds its own: same row ranges, so map by range
        by_range = {(g0, g1): bs[id(bw)] for g0, g1, bw in groups}
        return (dY_below, {id(bw): by_range[(g0, g1)] for g0, g1, bw in below["groups"]})

    def adapter(self, i, L):
        """token path of the lateral adapter in front of block i (its convolutions: train_conv.py)."""
        e, dX, Mv, conv, grads = self.e, self.dX, self.Mv, self.conv, self.grads
        ad = L["adapter"]
        a = e.adapters[ad["j"]]
        dsum = torch.empty(Mv, self.D, dtype=F32, device=self.dev)
        part, _ = hip.layernorm_bwd(ad["sum"], dX[:Mv], a["ln"].g, dsum, Mv, accumulate=False, fold=False)
        self.ln_param_grads(part, f"visual.transformer.parallel_lateral_adapter.{ad['j']}.ln_adapt")
        # adapter convs + parallel stage j (train_conv.py) -> the gradient matrix and depthwise filter of the token path
        # (moving the frozen walk's chain -- bandwidth-bound, nothing on the critical path reads its products -- to the lane
        #  stream was measured: 88.5-88.9 -> 91.0-91.1 ms per step, its kernels take CUs from the dgrad GEMMs)
        dgrid, dww = conv.adapter(grads, ad["j"], dsum, ad["x_pre"])
        hip.adapter_dx(dgrid, dww, dX[:Mv], self.Bi, e.Lv, e.g, e.usecls)

    def embed_bwd(self):
        """Token and text positional embedding gradients as ONE flat tensor (on_lane's contract), from the text rows of dX."""
        e, sv, D, Mv = self.e, self.sv, self.D, self.Mv
        dX_text, tok_ids, sv_cap, n_live, ne = self.dX[Mv:self.M], sv["tok"], sv["cap"], sv["Mt_live"], e.emb.numel()
        flat = torch.zeros(ne + e.Lt * D, dtype=F32, device=self.dev)                     # one tensor: on_lane's contract
        # the positional embedding's gradient is a sum over the batch: a column sum in a fixed order (bitwise repeatable),
        # not the kernel's atomics; the token embedding's scatter-add stays atomic (captions share ids)
        if sv_cap is not None:
            # packed rows: scatter-add over the live rows, positional sums over the captions that have the position
            hip.embed_tokens_bwd_packed(tok_ids, dX_text[:n_live], sv_cap.cu, flat[:ne].view_as(e.emb), flat[ne:].view(e.Lt, D))
        elif dX_text.is_contiguous():
            hip.embed_tokens_bwd(tok_ids, dX_text, flat[:ne].view_as(e.emb), None)
            hip.colsum(dX_text.view(self.Bt, e.Lt * D), out=flat[ne:])
        else:
            hip.embed_tokens_bwd(tok_ids, dX_text, flat[:ne].view_as(e.emb), flat[ne:].view(e.Lt, D))
        return flat

    def fronts(self):
        """---- fronts: text embedding, image cls / positional embeddings, ln_pre -> dtok, the gradient of the image tokens in
        front of ln_pre (the stem's, or the patch weight's, input gradient)."""
        e, sv, grads, dX, D, Mv = self.e, self.sv, self.grads, self.dX, self.D, self.Mv
        # the text rows of dX are final here and nothing below reads the result: the scatter-add (0.67 ms of atomics at
        # batch 512) runs on the lane, beside the stem's backward
        ne = e.emb.numel()
        both = gradgemm.on_lane(self.embed_bwd, dX[Mv:self.M], sv["tok"], *([sv["cap"].cu] if sv["cap"] is not None else []))
        grads["token_embedding.weight"], grads["positional_embedding"] = both[:ne].view_as(e.emb), both[ne:].view(e.Lt, D)
        dtok = torch.empty(Mv, D, dtype=F32, device=self.dev)
        part, _ = hip.layernorm_bwd(sv["tok_pre"], dX[:Mv], e.ln_pre.g, dtok, Mv, accumulate=False, fold=False)
        self.ln_param_grads(part, "visual.ln_pre")
        dvpos = hip.colsum(dtok.view(self.Bi, e.Lv * D)).view(e.Lv, D)                      # sum over the batch
        grads["visual.positional_embedding"] = dvpos
        grads["visual.class_embedding"] = dvpos[0].clone()
        return dtok



class _Accumulators:
    """The persistent fp32 gradient accumulators of TrainStep.accumulate(): one arena, every tensor at a 256-byte boundary,
    one view per gradient key in the shape backward() returns it; msclip_grad_accumulate's table over them is built once."""

    def __init__(self, grads):
        self.keys = list(grads)
        self.shapes = {k: (tuple(t.shape), t.device) for k, t in grads.items()}
        dev = grads[self.keys[0]].device
        offs, total = [], 0
        for k in self.keys:
            offs.append(total)
            total += (grads[k].numel() + 63) // 64 * 64
        self.arena = torch.zeros(total, dtype=F32, device=dev)
        self.views = {k: self.arena[o:o + grads[k].numel()].view(grads[k].shape) for k, o in zip(self.keys, offs)}
        self.plan = hip.AccumulatePlan([self.views[k].view(-1) for k in self.keys])

    def add(self, grads, mode):
        """mode 0: accumulators = grads (the first chunk); 1: += grads.  The few gradients that arrive as permuted views
        (depthwise adapter weights) are made contiguous first, as _adamw_plan does."""
        assert len(grads) == len(self.keys)
        flat = [grads[k] if grads[k].is_contiguous() else grads[k].contiguous() for k in self.keys]
        self.plan.run(flat, mode)


class _EmaShadow:
    """The shadow weights of TrainStep(ema_decay=...): one fp32 arena, every tensor at a 256-byte boundary, one view per entry
    of model.named_parameters() (one per Parameter object: the text-tower aliases of the shared tensors are not separate
    entries; buffers are not shadowed), each a copy of its parameter at construction.  msclip_ema_multi's table over
    (shadow, parameter) is built once: neither side moves."""

    def __init__(self, model):
        named = list(model.named_parameters())
        dev = named[0][1].device
        offs, total = [], 0
        for _, p in named:
            assert p.dtype == F32 and p.is_contiguous() and p.device == dev, (p.dtype, p.is_contiguous(), p.device)
            offs.append(total)
            total += (p.numel() + 63) // 64 * 64
        with torch.no_grad():
            self.arena = torch.zeros(total, dtype=F32, device=dev)
            self.views = {k: self.arena[o:o + p.numel()].view(p.shape) for (k, p), o in zip(named, offs)}
            self.params = {k: p for k, p in named}
            for k, p in named:
                self.views[k].copy_(p.detach())
        self.plan = hip.EmaPlan([v.view(-1) for v in self.views.values()], [p.data.view(-1) for _, p in named])

    def swap(self):
        """Exchange the values of every parameter and its shadow, in place on both sides."""
        with torch.no_grad():
            for k, p in self.params.items():
                s = self.views[k]
                live = p.detach().clone()
                p.copy_(s)
                s.copy_(live)

    def load(self, states):
        """`states`: {name: tensor} of a checkpoint's 'ema_shadow_states', the same names and shapes as the shadows."""
        if set(states) != set(self.views):
            odd = sorted(set(states) ^ set(self.views))
            raise KeyError(f"'ema_shadow_states' does not name this model's parameters (first differences: {odd[:4]})")
        with torch.no_grad():
            for k, v in self.views.items():
                if tuple(states[k].shape) != tuple(v.shape):
                    raise ValueError(f"'ema_shadow_states'[{k!r}] has shape {tuple(states[k].shape)}, the parameter {tuple(v.shape)}")
                v.copy_(states[k])


def world_average_(grads):
    """In-place rank mean of a gradient dict produced with backward(reduce=False) (what step(world_average=True) runs): one
    all-reduce per tensor.  Non-contiguous entries (the conv side's depthwise weight gradients are transposed views,
    train_conv.py) are replaced by dense copies first: NCCL / gloo reject strided tensors."""
    if C.comm.world_size <= 1:
        return grads
    for k in list(grads):
        g = grads[k]
        if not g.is_contiguous():
            g = grads[k] = g.contiguous()
        dist.all_reduce(g)
        g /= C.comm.world_size
    return grads


def param_groups(model, lr, lr_share, wd, wd_share, without_wd=("bn", "bias", "ln")):
    """(name, parameter, lr, weight_decay) for every parameter of the slice, following the reference's yaml: shared
    attention / MLP tensors use CUSTOM.LR_SHARE / WD_SHARE, everything else TRAIN.LR / TRAIN.WD; no decay for the
    TRAIN.WITHOUT_WD_LIST keywords -- 'bn' = parameters of BatchNorm modules (whatever their name: the stem's
    `downsample.1` is one), 'ln' = parameters of LayerNorm modules, 'bias' = names ending in 'bias' -- and for every
    name that CONTAINS an entry of model.no_weight_decay() (M.py:2950-2956: 'positional_embedding' covers
    visual.positional_embedding, 'token_embedding' covers token_embedding.weight)."""
    m = model
    norm_params = set()
    for mod in m.modules():
        if (isinstance(mod, torch.nn.BatchNorm2d) and "bn" in without_wd) or \
           (isinstance(mod, torch.nn.LayerNorm) and "ln" in without_wd):
            norm_params.update(id(p) for p in mod.parameters(recurse=False))
    shared = set()
    if m.share_from_layer is not None:
        for i in range(max(m.share_from_layer, 1), len(m.visual.transformer.resblocks)):
            shared.update(f"visual.transformer.resblocks.{i}.{leaf}" for leaf in _LEAVES)
    nodecay = set(m.no_weight_decay())
    params = dict(m.named_parameters())
    out = []
    for k, p in params.items():
        plr = lr_share if (k in shared and lr_share is not None) else lr
        pwd = wd_share if (k in shared and wd_share is not None) else wd
        if id(p) in norm_params or ("bias" in without_wd and k.endswith("bias")) or any(t in k for t in nodecay):
            pwd = 0.0
        out.append((k, p, plr, pwd))
    return out


def _optimizer_state_dict(ts):
    """TrainStep's AdamW state in torch.optim.AdamW's state_dict layout (parameter indices in named_parameters order, one
    param_group per distinct (lr, weight_decay)): what the reference's `save_checkpoint_on_master` stores under
    'optimizer' (lib/utils/utils.py:177-183)."""
    groups, index = {}, {}
    state = {}
    guard = getattr(ts, "nonfinite", None) is not None      # with the guard: 'step' is the applied count, 'msclip' says how many were skipped
    skipped = int(ts.skipped_steps) if guard else 0
    extra = {"skipped_steps": skipped} if guard else {}
    for i, (k, p, lr, wd) in enumerate(ts.param_groups()):
        index[k] = i
        groups.setdefault((lr, wd), []).append(i)
        st = ts.state.get(k)
        if st is not None:
            state[i] = {"step": torch.tensor(float(ts.steps - skipped)), "exp_avg": st[0].detach().cpu(), "exp_avg_sq": st[1].detach().cpu()}
    if getattr(ts, "optimizer", "adamw") == "lamb":       # timm Lamb's group keys; the adamW dict is what it was before lamb existed
        pgs = [{"lr": lr, "weight_decay": wd, "bias_correction": True, "betas": tuple(ts.betas), "eps": ts.eps, "grad_averaging": True,
                "max_grad_norm": float(ts.clip_grad_norm) if ts.clip_grad_norm else None, "trust_clip": ts.trust_clip,
                "always_adapt": ts.always_adapt, "params": idx} for (lr, wd), idx in groups.items()]
        return {"state": state, "param_groups": pgs,
                "msclip": dict({"steps": ts.steps, "bn": ts.bn, "names": list(index), "optimizer": "lamb"}, **extra)}
    pgs = [{"lr": lr, "weight_decay": wd, "betas": tuple(ts.betas), "eps": ts.eps, "amsgrad": False, "params": idx}
           for (lr, wd), idx in groups.items()]
    return {"state": state, "param_groups": pgs, "msclip": dict({"steps": ts.steps, "bn": ts.bn, "names": list(index)}, **extra)}


def _check_optimizer_kind(opt, ts, path):
    """A checkpoint's moments belong to the optimizer that wrote them ('msclip'.'optimizer'; absent: adamw)."""
    kind = str(opt["msclip"].get("optimizer", "adamw")).lower()
    mine = getattr(ts, "optimizer", "adamw")
    if kind != mine:
        raise ValueError(f"{path} was written by TRAIN.OPTIMIZER {kind!r}, this TrainStep runs {mine!r}: the optimizer "
                         "state of one is not the other's")


def save_checkpoint(model, ts, path, step, model_name="", perf=0.0):
    """The reference's resumable checkpoint dict (lib/utils/utils.py:157-200): 'step', 'model', 'state_dict', 'perf',
    'optimizer', and with TrainStep(ema_decay=...) 'ema_shadow_states' = {parameter name: CPU tensor}, the reference's
    `ema_model.shadow` (utils.py:187-188); without EMA the file is what it was before the key existed.  With drop_path > 0 also
    'drop_path_rng_state', the state of the TrainStep's mask generator (absent otherwise).  'state_dict' holds the
    live weights: not to be called between ema_assign() and ema_resume().  Rank 0 only under N > 1."""
    ts._ema_live("save_checkpoint")
    if not C.comm.is_main_process():
        return
    out = {"step": step + 1, "model": model_name, "perf": perf,
           "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
           "optimizer": _optimizer_state_dict(ts)}
    if ts.ema_shadow is not None:
        out["ema_shadow_states"] = {k: v.detach().cpu() for k, v in ts.ema_shadow.items()}
    if ts._dp_gen is not None:                        # stochastic depth: the mask generator continues where it stopped
        out["drop_path_rng_state"] = ts._dp_gen.get_state()
    torch.save(out, path)


def resume_checkpoint(model, ts, path):
    """-> the step to continue from.  Loads the module (strict, aliases checked), the AdamW moments and the step count.
    With TrainStep(ema_decay=...) also the shadow weights from 'ema_shadow_states'; a checkpoint without that key is refused,
    as the reference asserts (lib/utils/utils.py:129-133).  Without EMA the key is ignored.  With drop_path > 0 the mask
    generator takes 'drop_path_rng_state'; where the key is absent (an older checkpoint) it is reseeded from drop_path_seed."""
    from .checkpoint import check_aliases, extract_state_dict
    ts._ema_live("resume_checkpoint")
    obj = torch.load(path, map_location="cpu", weights_only=False)
    _check_optimizer_kind(obj["optimizer"], ts, path)    # (before anything is loaded)
    if ts.ema_shadow is not None and "ema_shadow_states" not in obj:
        raise KeyError(f"{path} has no 'ema_shadow_states': it was written without TRAIN.EMA_DECAY, this TrainStep has "
                       f"ema_decay = {ts.ema_decay}")
    sd = extract_state_dict(obj)
    model.load_state_dict(sd, strict=True)
    check_aliases(model, sd)
    opt = obj["optimizer"]
    names = opt["msclip"]["names"]
    params = dict(model.named_parameters())
    ts.state = {}
    for i, st in opt["state"].items():
        p = params[names[int(i)]]
        ts.state[names[int(i)]] = (st["exp_avg"].to(p.device).contiguous(), st["exp_avg_sq"].to(p.device).contiguous())
    ts.steps = int(opt["msclip"]["steps"])
    skipped = int(opt["msclip"].get("skipped_steps", 0))  # written with the non-finite guard on
    if getattr(ts, "nonfinite", None) is not None:        # both counters; a verdict still in flight belongs to the replaced state
        ts._skip_base, ts._skip_seen, ts._skip_event, ts.last_skipped = skipped, 0, None, None
    else:
        ts.steps -= skipped                               # no guard here: the step count IS the bias corrections' exponent
    if ts.ema_shadow is not None:
        ts._ema.load(obj["ema_shadow_states"])
    if ts._dp_gen is not None:
        # a checkpoint written before the key existed (or without stochastic depth): the masks restart from the seed
        if "drop_path_rng_state" in obj:
            ts._dp_gen.set_state(obj["drop_path_rng_state"])
        else:
            ts._dp_gen.manual_seed(ts.drop_path_seed)
    ts._plan = None                                   # the cached optimizer table points at the moments just replaced
    ts.eng.refresh(force=True)
    return int(obj.get("step", ts.steps))


def from_config(model, config, bn="batch", drop_path_mode="sample"):
    """TrainStep with the reference yaml's optimizer block (experiments/model/b32.yaml:32-52 + the msclips overlays):
    TRAIN.OPTIMIZER (adamW, or lamb / timm with OPTIMIZER_ARGS.opt lamb -- optimizer_settings; anything else raises), TRAIN.LR / WD / WITHOUT_WD_LIST, TRAIN.OPTIMIZER_ARGS
    (betas / eps; absent => torch.optim.AdamW's defaults, what `AdamW(params, lr=..., weight_decay=..., **{})` gives),
    CUSTOM.LR_SHARE / WD_SHARE for the modality-shared tensors (already scaled with the world size by update_config,
    lib/config/default.py:299-304), TRAIN.CLIP_GRAD_NORM (global-norm clipping inside step(); 0.0 = off), TRAIN.EMA_DECAY
    (shadow weights updated inside step(); absent or 0.0 = off), MODEL.SPEC.VISION.DROP_PATH (stochastic depth on the vision
    blocks, one draw per image per branch unless drop_path_mode says "position"; absent or 0.0 = off), TRAIN.DETECT_ANOMALY /
    TRAIN.SKIP_NONFINITE (nonfinite_setting: the non-finite guard of step(); both absent or False = off).
    bn = "batch" (default): train-mode BatchNorm as the reference's modules run in train(); "frozen": running statistics."""
    settings = optimizer_settings(config)
    ts = TrainStep(model, bn=bn, ema_decay=ema_setting(config), drop_path=drop_path_setting(config), drop_path_mode=drop_path_mode,
                   nonfinite=nonfinite_setting(config), **settings)
    if "clip_grad_norm" not in settings:             # (lamb: already settled between CLIP_GRAD_NORM and OPTIMIZER_ARGS.max_grad_norm)
        ts.clip_grad_norm = float(config.TRAIN.get("CLIP_GRAD_NORM", 0.0) or 0.0)      # 0.0: off (lib/config/default.py:153)
    ts.schedule = lr_schedule(config)            # TRAIN.LR_SCHEDULER of the yaml (None when the config has none)
    return ts


class CosineSchedule:
    """TRAIN.LR_SCHEDULER {METHOD: 'timm', ARGS: {sched: 'cosine', ...}} of the reference yamls (experiments/model/b32.yaml:40-48;
    lib/config/default.py:306-308 adds ARGS.epochs = TRAIN.END_EPOCH and hands ARGS to timm's create_scheduler in the unreleased
    trainer).  timm's CosineLRScheduler stepped once per EPOCH (t_in_epochs), one cycle, no warm-up prefix:
        t <  warmup_epochs:  lr = warmup_lr + t * (base - warmup_lr) / warmup_epochs
        t <  epochs:         lr = min_lr + 0.5 * (base - min_lr) * (1 + cos(pi * t / epochs))
        t >= epochs:         lr = min_lr        (the cooldown_epochs run at min_lr; the run lasts epochs + cooldown_epochs)
    applied to every parameter group's own base rate (TRAIN.LR for the modality-specific tensors, CUSTOM.LR_SHARE for the shared)."""

    def __init__(self, epochs, warmup_epochs=0, warmup_lr=0.0, min_lr=0.0, cooldown_epochs=0, decay_rate=0.1):
        self.epochs, self.warmup_epochs, self.warmup_lr, self.min_lr = int(epochs), int(warmup_epochs), float(warmup_lr), float(min_lr)
        self.cooldown_epochs, self.decay_rate = int(cooldown_epochs), float(decay_rate)      # (decay_rate only acts on later cycles: one cycle here)
        self.total_epochs = self.epochs + self.cooldown_epochs

    def lr_at(self, base, epoch):
        import math
        t = int(epoch)
        if t < self.warmup_epochs:
            return self.warmup_lr + t * (base - self.warmup_lr) / self.warmup_epochs
        if t < self.epochs:
            return self.min_lr + 0.5 * (base - self.min_lr) * (1.0 + math.cos(math.pi * t / self.epochs))
        return self.min_lr


def lr_schedule(config):
    """The scheduler block of a reference config (needs no GPU); None when TRAIN.LR_SCHEDULER is absent."""
    tr = config.TRAIN
    sch = tr.get("LR_SCHEDULER", None)
    if not sch or not sch.get("METHOD", None):
        return None
    if str(sch.METHOD) != "timm":
        raise NotImplementedError(f"TRAIN.LR_SCHEDULER.METHOD = {sch.METHOD!r}: the released configs use 'timm' (cosine)")
    a = dict(sch.get("ARGS", None) or {})
    if str(a.get("sched", "cosine")) != "cosine":
        raise NotImplementedError(f"TRAIN.LR_SCHEDULER.ARGS.sched = {a.get('sched')!r}: only timm's cosine schedule is implemented")
    # the reference's update_config sets ARGS.epochs = TRAIN.END_EPOCH unconditionally (lib/config/default.py:306-311): the yaml's
    # END_EPOCH wins over an `epochs` key under ARGS
    epochs = int(tr.get("END_EPOCH", 0) or 0) or int(a.get("epochs", 0) or 0)
    warm = int(a.get("warmup_epochs", 0) or 0)
    if epochs <= 0 or epochs <= warm:
        raise ValueError(f"TRAIN.LR_SCHEDULER: the cosine schedule needs TRAIN.END_EPOCH ({epochs}) > ARGS.warmup_epochs ({warm})")
    return CosineSchedule(epochs=epochs, warmup_epochs=warm,
                          warmup_lr=a.get("warmup_lr", 0.0), min_lr=a.get("min_lr", 0.0),
                          cooldown_epochs=a.get("cooldown_epochs", 0), decay_rate=a.get("decay_rate", 0.1))


def ema_setting(config):
    """TRAIN.EMA_DECAY of a reference config as TrainStep's `ema_decay` (needs no GPU): None when the key is absent or 0.0,
    the reference's default (lib/config/default.py:146; its run name carries 'ema<decay>' only when > 0, :268-270)."""
    return float(config.TRAIN.get("EMA_DECAY", 0.0) or 0.0) or None


def nonfinite_setting(config):
    """TrainStep's `nonfinite` from a reference config (needs no GPU): TRAIN.DETECT_ANOMALY True (lib/config/default.py:151; the
    unreleased trainer's switch for torch's anomaly detection) -> "raise"; else TRAIN.SKIP_NONFINITE True (this
    project's key) -> "skip"; else None."""
    if bool(config.TRAIN.get("DETECT_ANOMALY", False)):
        return "raise"
    return "skip" if bool(config.TRAIN.get("SKIP_NONFINITE", False)) else None


def nonfinite_names(partials, names_and_sizes):
    """The chunk -> parameter map of the norm's table as a pure function (CPU tensors are fine).  partials: the fp32 partial sums
    of squares of msclip_grad_sumsq, one per started 32 K-element chunk; names_and_sizes: [(parameter name, element count)] in
    the table's order, one entry per Parameter object (the joined pieces of in_proj are one entry).  -> the names whose chunks
    hold a NaN or an Inf, in that order."""
    chunk = hip.CLIP_CHUNK
    total = sum((n + chunk - 1) // chunk for _, n in names_and_sizes)
    if partials.dim() != 1 or partials.numel() != total:
        raise ValueError(f"partials: {tuple(partials.shape)}, the table has {total} chunks")
    bad = ~torch.isfinite(partials)
    out, c = [], 0
    for name, n in names_and_sizes:
        k = (n + chunk - 1) // chunk
        if k and bool(bad[c:c + k].any()):
            out.append(name)
        c += k
    return out


def drop_path_setting(config):
    """MODEL.SPEC.VISION.DROP_PATH of a reference config (M.py:3188) as TrainStep's `drop_path` (needs no GPU): 0.0 when the key
    is absent -- an explicit "off", so that the config and not a stale model attribute decides; a rate outside [0, 1) raises."""
    p = float(config.MODEL.SPEC.VISION.get("DROP_PATH", 0.0) or 0.0)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"MODEL.SPEC.VISION.DROP_PATH = {p!r}: a drop rate in [0, 1)")
    return p


def drop_path_table(keep_draws, Bi, Lv, M, mode, keep):
    """The fp32 row-scale tables of the launches that carry stochastic depth, from one set of Bernoulli draws (pure tensor code:
    runs wherever keep_draws lives, CPU included).
    keep_draws: bool [vision blocks, 2 (attention branch, MLP branch), Bi] in mode "sample" -- one draw per image -- or
    [vision blocks, 2, Lv] in mode "position" -- one draw per token position, shared by all images (timm's DropPath on the
    reference's sequence-first blocks).  -> fp32 [vision blocks, 2, M]: row b * Lv + l of the token matrix (image b, token l)
    holds 1 / keep where its draw kept the branch and 0 where it dropped it; rows Bi * Lv .. M -- the text tokens, sized to the
    launch's upper bound M so that a packed caption batch needs nothing more -- hold 1."""
    if mode not in DROP_PATH_MODES:
        raise ValueError(f"mode = {mode!r}: one of {DROP_PATH_MODES}")
    n = Bi if mode == "sample" else Lv
    if keep_draws.dtype != torch.bool or keep_draws.dim() != 3 or keep_draws.shape[1] != 2 or keep_draws.shape[2] != n:
        raise ValueError(f"keep_draws: bool [blocks, 2, {n}] in mode {mode!r}, got {keep_draws.dtype} {tuple(keep_draws.shape)}")
    if not 0.0 < keep <= 1.0 or M < Bi * Lv:
        raise ValueError(f"keep = {keep!r} (0 < keep <= 1), M = {M} (>= {Bi * Lv} image rows)")
    nb = keep_draws.shape[0]
    per = keep_draws[:, :, :, None].expand(nb, 2, Bi, Lv) if mode == "sample" else keep_draws[:, :, None, :].expand(nb, 2, Bi, Lv)
    out = torch.ones(nb, 2, M, dtype=F32, device=keep_draws.device)
    img = out[:, :, :Bi * Lv].view(nb, 2, Bi, Lv)
    img.copy_(torch.where(per, torch.tensor(1.0 / keep, dtype=F32, device=keep_draws.device),
                          torch.zeros((), dtype=F32, device=keep_draws.device)))
    return out


def optimizer_settings(config):
    """The optimizer block of a reference config as TrainStep keyword arguments (needs no GPU).
    TRAIN.OPTIMIZER adamW: OPTIMIZER_ARGS betas / eps (torch.optim.AdamW's defaults) and lr (ignored: TRAIN.LR rules).
    TRAIN.OPTIMIZER lamb, or timm with OPTIMIZER_ARGS.opt lamb (lib/config/default.py:313-314; both case-insensitive): timm
    Lamb's keys -- betas / opt_betas, eps / opt_eps (default 1e-6), trust_clip, always_adapt, max_grad_norm, and
    bias_correction / grad_averaging, which must be true.  max_grad_norm becomes clip_grad_norm where TRAIN.CLIP_GRAD_NORM is 0;
    both set and different is a ValueError; neither means no clipping (timm's own default of 1.0 is NOT applied: the
    reference's CLIP_GRAD_NORM 0.0 is).  For lamb the result carries optimizer / trust_clip / always_adapt / clip_grad_norm;
    for adamW it is what it was before lamb existed."""
    tr, cu = config.TRAIN, config.CUSTOM
    opt = str(tr.get("OPTIMIZER", "sgd"))
    oa = dict(tr.get("OPTIMIZER_ARGS", None) or {})
    kind = opt.lower()
    if kind == "timm":
        kind = str(oa.pop("opt", "")).lower()
        if kind != "lamb":
            raise NotImplementedError(f"TRAIN.OPTIMIZER = 'timm' with OPTIMIZER_ARGS.opt = {kind!r}: of timm's optimizers this "
                                      "build implements lamb only")
    if kind not in ("adamw", "lamb"):
        raise NotImplementedError(f"TRAIN.OPTIMIZER = {opt!r}: this build implements adamW (the released MS-CLIP-S configs' "
                                  "optimizer, experiments/model/b32.yaml:48) and lamb")
    base = dict(lr=tr.LR, lr_share=cu.get("LR_SHARE", None) or None, wd=tr.WD, wd_share=cu.get("WD_SHARE", None) or None)
    without_wd = tuple(tr.get("WITHOUT_WD_LIST", ()) or ())
    oa.pop("lr", None)
    if kind == "adamw":
        betas = tuple(oa.pop("betas", (0.9, 0.999)))
        eps = float(oa.pop("eps", 1e-8))
        if oa:
            raise NotImplementedError(f"TRAIN.OPTIMIZER_ARGS keys {sorted(oa)} are not implemented")
        return dict(base, betas=betas, eps=eps, without_wd=without_wd)

    def either(a, b, default):
        if a in oa and b in oa and oa[a] != oa[b]:
            raise ValueError(f"TRAIN.OPTIMIZER_ARGS.{a} = {oa[a]!r} and .{b} = {oa[b]!r} disagree")
        va, vb = oa.pop(a, None), oa.pop(b, None)
        return default if va is None and vb is None else (vb if va is None else va)

    betas = tuple(either("betas", "opt_betas", (0.9, 0.999)))
    eps = float(either("eps", "opt_eps", OPTIMIZERS["lamb"]))
    for key in ("bias_correction", "grad_averaging"):
        if not bool(oa.pop(key, True)):
            raise NotImplementedError(f"TRAIN.OPTIMIZER_ARGS.{key} = False is not implemented (lamb runs with both on)")
    trust_clip, always_adapt = bool(oa.pop("trust_clip", False)), bool(oa.pop("always_adapt", False))
    own = float(oa.pop("max_grad_norm", 0.0) or 0.0)
    clip = float(tr.get("CLIP_GRAD_NORM", 0.0) or 0.0)
    if own and clip and own != clip:
        raise ValueError(f"TRAIN.CLIP_GRAD_NORM = {clip!r} and TRAIN.OPTIMIZER_ARGS.max_grad_norm = {own!r} disagree: set one")
    if oa:
        raise NotImplementedError(f"TRAIN.OPTIMIZER_ARGS keys {sorted(oa)} are not implemented")
    return dict(base, betas=betas, eps=eps, without_wd=without_wd, optimizer="lamb", trust_clip=trust_clip,
                always_adapt=always_adapt, clip_grad_norm=clip or own)
