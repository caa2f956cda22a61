"""LAMB as the training step specifies it (timm's Lamb with bias_correction and grad_averaging), restated in fp64 torch for the
tests.  A test helper: nothing here comes from msclip_amd.

For every tensor w with gradient g, moments m, v, step t (from 1), its lr and wd:
    g' = g * coef
    m  = b1 m + (1 - b1) g',   v = b2 v + (1 - b2) g'^2
    u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd w
    r  = ||w|| / ||u||  if (wd != 0 or always_adapt) and ||w|| > 0 and ||u|| > 0, else 1    (NaN fails both comparisons)
    r  = min(r, 1)      if trust_clip
    w  = w - lr r u
"""
import torch

F64 = torch.float64


def clip_coef(grads, max_norm):
    """coef = min(1, max_norm / (norm + 1e-6)) over the global L2 norm of `grads` (torch.nn.utils.clip_grad_norm_'s)."""
    norm = torch.sqrt(sum((g.to(F64) ** 2).sum() for g in grads.values()))
    return float(min(1.0, max_norm / (float(norm) + 1e-6))), float(norm)


def lamb_step(params, grads, state, step, lr, wd, betas=(0.9, 0.999), eps=1e-6, coef=1.0, trust_clip=False, always_adapt=False):
    """One step.  params / grads: {name: tensor} (any float dtype; read as fp64, not written); state: {name: (m, v)} of fp64
    tensors, REPLACED with the new moments (a missing name starts from zeros); lr / wd: a float or {name: float}.
    -> {name: dict(w=new parameter, delta=w_new - w, u=u, r=the ratio applied, raw=||w|| / ||u|| by the rule without the
    wd / always_adapt condition, wn=||w||, un=||u||)}, all fp64."""
    b1, b2 = betas
    out = {}
    for k, w in params.items():
        w = w.detach().to(F64)
        g = grads[k].detach().to(F64).reshape(w.shape) * coef
        m, v = state.get(k, (torch.zeros_like(w), torch.zeros_like(w)))
        m = b1 * m.to(F64) + (1 - b1) * g
        v = b2 * v.to(F64) + (1 - b2) * g * g
        state[k] = (m, v)
        lr_k = lr[k] if isinstance(lr, dict) else lr
        wd_k = wd[k] if isinstance(wd, dict) else wd
        u = (m / (1 - b1 ** step)) / (torch.sqrt(v / (1 - b2 ** step)) + eps) + wd_k * w
        wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
        raw = wn / un if bool(wn > 0) and bool(un > 0) else torch.ones((), dtype=F64)
        if trust_clip:
            raw = torch.clamp(raw, max=1.0)
        r = raw if (wd_k != 0 or always_adapt) else torch.ones((), dtype=F64)
        delta = -lr_k * r * u
        out[k] = dict(w=w + delta, delta=delta, u=u, r=r, raw=raw, wn=wn, un=un)
    return out
