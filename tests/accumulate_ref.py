"""Reference for TrainStep.accumulate (an ordinary helper module: no tests, no fixtures).

chunked_oracle_gradients() follows oracle/autograd.py::oracle_gradients -- same leaves, same aliasing of the shared tensors,
same loss -- but runs the image tower once per chunk, so that train-mode BatchNorm (Arch.bn_train) normalises every chunk
with its OWN batch statistics, as K ranks of the reference holding one chunk each would; the chunks' features are
concatenated and ONE symmetric cross-entropy over all N pairs is differentiated.  The text tower has no BatchNorm: it runs
once over all captions.  Only the oracle's public functions are used.  With one chunk this is oracle_gradients
(tests/test_accumulate_cpu.py pins that); with frozen statistics the chunking changes nothing but fp32 summation order."""
import dataclasses

import torch

from oracle import msclip_oracle as O
from oracle.autograd import parameter_aliases


def chunk_starts(sizes):
    starts = [0]
    for b in sizes:
        starts.append(starts[-1] + int(b))
    return starts


def chunked_oracle_gradients(model_or_sd, arch, img, tok, sizes, bn_train=False, autocast_bf16=False, aliases=None,
                             live_chunks=None):
    """({parameter name: full fp32 gradient}, loss) of the N-pair loss with the image tower run chunk by chunk.
    sizes: the chunk sizes (their sum = the batch).  live_chunks: None, or the chunks whose towers are differentiated -- the
    features of the others are constants (tests use it to build the defect "one chunk's gradient dropped")."""
    if isinstance(model_or_sd, torch.nn.Module):
        aliases = parameter_aliases(model_or_sd)
        sd = model_or_sd.state_dict()
    else:
        sd = model_or_sd
        if aliases is None:
            raise ValueError("a state_dict needs the alias map of its model (parameter_aliases)")
    starts = chunk_starts(sizes)
    assert starts[-1] == img.shape[0] == tok.shape[0], (sizes, img.shape, tok.shape)
    arch = dataclasses.replace(arch, bn_train=bn_train)
    leaves = {}
    bound = {k: v.detach().float().cpu() for k, v in sd.items()}                  # buffers (running statistics) stay constants
    for k, first in aliases.items():
        if first not in leaves:
            leaves[first] = bound[first].clone().requires_grad_(True)
        bound[k] = leaves[first]
    img, tok = img.detach().float().cpu(), tok.detach().cpu()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast_bf16):
        fi = [O.encode_image(img[a:b], bound, arch) for a, b in zip(starts, starts[1:])]
        ft = O.encode_text(tok, bound, arch)
        ft = [ft[a:b] for a, b in zip(starts, starts[1:])]
        if live_chunks is not None:
            fi = [f if k in live_chunks else f.detach() for k, f in enumerate(fi)]
            ft = [f if k in live_chunks else f.detach() for k, f in enumerate(ft)]
        loss = O.contrastive_loss(O.clip_logits(torch.cat(fi), torch.cat(ft), bound["logit_scale"]).float())
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    out = {k: (torch.zeros_like(leaves[k]) if g is None else g.detach().float()) for k, g in zip(names, grads)}
    return out, float(loss.item())


def in_chunk_mean(model_or_sd, arch, img, tok, sizes, **kw):
    """What summing K ordinary steps and dividing by K computes: the mean of the chunks' own losses / gradients, every pair
    against the negatives of its own chunk only.  -> (gradients, mean loss)."""
    starts = chunk_starts(sizes)
    total, losses = None, []
    for a, b in zip(starts, starts[1:]):
        g, l = chunked_oracle_gradients(model_or_sd, arch, img[a:b], tok[a:b], [b - a], **kw)
        losses.append(l)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    K = len(sizes)
    return {k: v / K for k, v in total.items()}, sum(losses) / K
