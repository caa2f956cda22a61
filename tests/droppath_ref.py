"""Stochastic depth (MODEL.SPEC.VISION.DROP_PATH) on the CPU oracle -- TEST INFRASTRUCTURE, an ordinary helper module (no tests,
no fixtures).

oracle.msclip_oracle.encode_image takes a stand-in for residual_block; block_fn() below is that block with timm's DropPath
(x * r / keep, r the replayed Bernoulli draw) on both branch outputs of every VISION block (M.py:801, 1027-1028); the text tower
runs the oracle's own block (the reference builds it without the argument, M.py:2774-2783).  droppath_gradients() restates the
~20 lines of oracle/autograd.py::oracle_gradients around it.  tests/test_droppath_cpu.py pins block_fn in "position" mode against
the imported reference module with a replaying DropPath stub.

Masks: bool [vision blocks that run, 2 (attention branch, MLP branch), n]; n = images in mode "sample" (one draw per image), tokens
per image in mode "position" (one draw per token position, shared by the batch: what timm computes on the reference's
sequence-first blocks)."""
import dataclasses

import torch

from oracle import msclip_oracle as O


def vision_slots(arch):
    """Indices of the vision blocks that run (slot 0 is the conv stem unless the patch conv tokenises)."""
    return list(range(0 if arch.patch_conv else 1, arch.vision_layers))


def mask_shape(arch, batch, mode):
    return (len(vision_slots(arch)), 2, batch if mode == "sample" else arch.grid * arch.grid + 1)


def mixed_masks(arch, batch, mode, seed=0):
    """Deterministic masks in which EVERY vision block drops at least one draw and keeps at least one, in both branches."""
    nb, _, n = mask_shape(arch, batch, mode)
    assert n >= 2
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(nb, 2, n, generator=g) < 0.6
    for b in range(nb):
        for k in range(2):
            i = (b + 3 * k) % n
            m[b, k, i], m[b, k, (i + 1) % n] = False, True
    assert bool(m.any(-1).all()) and bool((~m).any(-1).all())
    return m


def block_fn(masks, mode, keep, arch, bias_unscaled=False):
    """The residual block encode_image calls for every vision slot, with the replayed draws.
    bias_unscaled=True plants a DEFECT for the tests' negative: the forward is unchanged, but out_proj.bias / c_proj.bias receive
    the gradient sum_rows dX[row] instead of sum_rows s[row] dX[row] -- a backward that forgot the scale in its bias sums."""
    first = vision_slots(arch)[0]
    assert tuple(masks.shape) == (len(vision_slots(arch)), 2, masks.shape[2]) and masks.dtype == torch.bool

    def scale(vi, k, x):
        r = masks[vi, k].to(torch.float32) / keep
        assert r.numel() == (x.shape[0] if mode == "sample" else x.shape[1]), (r.shape, x.shape, mode)
        return r[:, None, None] if mode == "sample" else r[None, :, None]

    def branch(f, sd, bias_key, s):
        if not bias_unscaled:
            return s * f(sd)
        b = sd[bias_key]
        return s * f({**sd, bias_key: b.detach()}) + (b - b.detach())       # value s * f; d / d bias = the unscaled row sum

    def fn(x, sd, p, heads, mask=None):
        assert p.startswith("visual.transformer.resblocks."), p
        vi = int(p.rsplit(".", 1)[1]) - first
        x = x + branch(lambda d: O.attention(O.layer_norm(x, d[p + ".ln_1.weight"], d[p + ".ln_1.bias"]), d, p + ".attn", heads, mask),
                       sd, p + ".attn.out_proj.bias", scale(vi, 0, x))
        x = x + branch(lambda d: O.mlp(O.layer_norm(x, d[p + ".ln_2.weight"], d[p + ".ln_2.bias"]), d, p + ".mlp"),
                       sd, p + ".mlp.c_proj.bias", scale(vi, 1, x))
        return x
    return fn


def droppath_forward(sd, arch, img, tok, masks, mode, keep, bn_train=False, autocast_bf16=False):
    """-> (image features, text features, loss) of the fp32 oracle with the replayed draws (autocast_bf16: of the same graph under
    torch.autocast(bfloat16), the yardstick of what bf16 GEMM operands cost)."""
    arch = dataclasses.replace(arch, bn_train=bn_train)
    sd = {k: v.detach().float().cpu() for k, v in sd.items()}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast_bf16):
        fi = O.encode_image(img.float().cpu(), sd, arch, block_fn=block_fn(masks.cpu(), mode, keep, arch)).float()
        ft = O.encode_text(tok.cpu(), sd, arch).float()
        loss = O.contrastive_loss(O.clip_logits(fi, ft, sd["logit_scale"]).float())
    return fi, ft, float(loss)


def droppath_gradients(sd, arch, img, tok, masks, mode, keep, aliases, bn_train=False, autocast_bf16=False, bias_unscaled=False):
    """oracle.autograd.oracle_gradients with the vision blocks of block_fn: ({parameter name: full fp32 gradient}, loss)."""
    arch = dataclasses.replace(arch, bn_train=bn_train)
    leaves = {}
    bound = {k: v.detach().float().cpu() for k, v in sd.items()}
    for k, first in aliases.items():
        if first not in leaves:
            leaves[first] = bound[first].clone().requires_grad_(True)
        bound[k] = leaves[first]
    img, tok = img.detach().float().cpu(), tok.detach().cpu()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast_bf16):
        fi = O.encode_image(img, bound, arch, block_fn=block_fn(masks.cpu(), mode, keep, arch, bias_unscaled=bias_unscaled))
        ft = O.encode_text(tok, bound, arch)
        loss = O.contrastive_loss(O.clip_logits(fi, ft, bound["logit_scale"]).float())
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    out = {k: (torch.zeros_like(leaves[k]) if g is None else g.detach().float()) for k, g in zip(names, grads)}
    return out, float(loss.item())
