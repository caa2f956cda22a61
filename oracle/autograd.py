"""Autograd through the CPU oracle  --  TEST INFRASTRUCTURE, NOT PRODUCT (see oracle/msclip_oracle.py).

oracle_gradients() differentiates contrastive_loss(forward(image, text)) of the plain-torch oracle and returns EVERY element of
every parameter's gradient, for any batch and seed.  The modality-shared tensors (one Parameter object under a visual.* and a
text-tower name, M.py:2808-2830) are ONE leaf bound under all their state_dict names, so their gradient is the sum over both
towers, as in the reference; it is returned under the first name of named_parameters(remove_duplicate=False), which is the name
tools/make_golden.py::grads_fixture stores it under (325 tensors for the B/32 and B/16 configs, 406 for L/14).

PINNING: tests/test_oracle_autograd_cpu.py checks these gradients against autograd of the REAL reference, fixture by fixture
(tests/golden/*.grads*.npz: loss, every stored 64-point sample and abs-mean, every tensor stored in full), in eval and in
train-mode BatchNorm.  That agreement (fp32 rounding) is what licenses tests/test_gpu_train_full.py to use this file as the
reference for the elements the fixtures do not hold.

autocast_bf16=True runs the same graph under torch.autocast(bfloat16): the gradients a correct implementation with bf16 GEMM
operands gives.  Its distance from the fp32 run is the YARDSTICK of tests/gradcheck.py -- the size of error that is precision,
not a defect."""
import dataclasses
from typing import Dict, Tuple

import torch

from . import msclip_oracle as O


def parameter_aliases(model) -> Dict[str, str]:
    """{every parameter name: the name its Parameter object is first listed under} (shared tensors: the visual.* name)."""
    first, out = {}, {}
    for k, p in model.named_parameters(remove_duplicate=False):
        out[k] = first.setdefault(id(p), k)
    return out


def oracle_gradients(model_or_sd, arch: O.Arch, img: torch.Tensor, tok: torch.Tensor, bn_train: bool = False,
                     autocast_bf16: bool = False, aliases: Dict[str, str] = None,
                     towers: Tuple[str, ...] = ("image", "text")) -> Tuple[Dict[str, torch.Tensor], float]:
    """({parameter name: full fp32 gradient}, loss) of the symmetric CE of the oracle's logits on (img, tok).

    model_or_sd: the nn.Module (its state_dict and alias map are taken) or a state_dict with `aliases` from
    parameter_aliases() of a module of the same configuration.  bn_train: BatchNorm with batch statistics (Arch.bn_train).
    towers: which towers the loss is differentiated through -- ("image",) takes the text features as constants, so that a
    shared tensor receives the image tower's share only (tests use it to build the defect "one tower's share left out")."""
    if isinstance(model_or_sd, torch.nn.Module):
        aliases = parameter_aliases(model_or_sd)
        sd = model_or_sd.state_dict()
    else:
        sd = model_or_sd
        if aliases is None:
            raise ValueError("a state_dict needs the alias map of its model (parameter_aliases)")
    arch = dataclasses.replace(arch, bn_train=bn_train)
    leaves = {}
    bound = {k: v.detach().float().cpu() for k, v in sd.items()}                  # buffers (running statistics) stay constants
    for k, first in aliases.items():
        if first not in leaves:
            leaves[first] = bound[first].clone().requires_grad_(True)
        bound[k] = leaves[first]
    img, tok = img.detach().float().cpu(), tok.detach().cpu()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast_bf16):
        fi = O.encode_image(img, bound, arch)
        ft = O.encode_text(tok, bound, arch)
        if "image" not in towers:
            fi = fi.detach()
        if "text" not in towers:
            ft = ft.detach()
        loss = O.contrastive_loss(O.clip_logits(fi, ft, bound["logit_scale"]).float())
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    out = {k: (torch.zeros_like(leaves[k]) if g is None else g.detach().float()) for k, g in zip(names, grads)}
    return out, float(loss.item())
