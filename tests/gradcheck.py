"""Full-tensor gradient metrics and their bounds, shared by tests/test_gpu_train_full.py (TrainStep on the GPU against the
oracle's autograd) and tests/test_gradcheck_cpu.py (the same assertions must catch planted defects).  An ordinary module: no
fixtures, no pytest hooks.

Three gradient sets per case, all {parameter name: full tensor}:
  ref   autograd of the fp32 oracle (oracle/autograd.py; = the reference's autograd, tests/test_oracle_autograd_cpu.py);
  yard  the same oracle under torch.autocast(bfloat16): what a CORRECT implementation with bf16 operands gives -- the yardstick;
  got   the implementation under test.
measure(x, ref) is applied to got and to yard alike; violations() bounds got's figures by yard's, never by anything got
itself produces.

Metrics, on every element of every tensor:
  block   the tensor viewed as [dim0, rest] (1-D: one column) is cut into blocks of 64 rows and, separately, into blocks of 64
          columns; per block ||x - ref|| / max(||ref||, 0.25 * rms block norm of that cut); the tensor's value is the worst block
          of both cuts.  A zeroed or mis-scaled head, a ragged tile tail, a dropped tower's share each own a block; the floor
          keeps blocks that are zero by symmetry (the k part of every in_proj bias) from dividing noise by noise.
  cos     cosine over the whole tensor (every tensor of more than one element).
  support (token_embedding.weight, positional_embedding) the rows ref leaves exactly zero -- ids absent from the batch, positions
          behind the longest caption -- and the worst per-row relative L2 error over the other rows.
"""
import numpy as np
import torch

BLOCK = 64
LNB = ("ln_1.bias", "ln_2.bias", "ln_final.bias", "ln_post.bias", "ln_pre.bias", "ln_adapt.bias")
CONV_SIDE = ("resblocks.0.conv1", "resblocks.0.bn1", "resblocks.0.resnet_stage", "resblocks.0.last_conv", "parallel_branch_v",
             "top2bottom", "bottom_dw_conv")                        # tests/test_gpu_train.py's classes
SUPPORT_KEYS = ("token_embedding.weight", "positional_embedding")
CLASSES = ("token", "lnb", "conv")
MEDIAN_FACTOR, MEDIAN_MARGIN = 1.25, 5e-3                           # the margins of the sampled tests (test_gpu_train.py)
WORST_MARGIN, COS_MARGIN, OWN_MARGIN = 4e-2, 5e-3, 2e-2
R_MAX = 2.0


def tensor_class(k):
    """"scalar" (logit_scale: one number, a sum of cancelling terms; bounded by its own yardstick as in test_gpu_train.py, and kept
    out of the token side's class figures, which it would otherwise loosen), "lnb", "conv" or "token"."""
    if k == "logit_scale":
        return "scalar"
    if k.endswith(LNB):
        return "lnb"
    if any(f in k for f in CONV_SIDE):
        return "conv"
    return "token"


def _as_matrix(t):
    t = t.detach().to("cpu", torch.float64)
    return t.reshape(t.shape[0], -1) if t.dim() >= 1 else t.reshape(1, 1)


def _cut(sq, dim):
    """Sums of a [R, C] matrix of squares over blocks of 64 along `dim` (all of the other dim): one value per block."""
    s = sq.sum(1 - dim)
    pad = (-s.numel()) % BLOCK
    if pad:
        s = torch.cat([s, s.new_zeros(pad)])
    return s.view(-1, BLOCK).sum(1)


def block_error(x, ref):
    x, ref = _as_matrix(x), _as_matrix(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    d2, r2 = (x - ref).square(), ref.square()
    worst = 0.0
    for dim in (0, 1):
        e, n = _cut(d2, dim).sqrt(), _cut(r2, dim)
        floor = 0.25 * n.mean().sqrt()
        den = torch.maximum(n.sqrt(), floor)
        q = torch.where(e > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))      # 0 / 0 (an all-zero tensor reproduced) is 0
        worst = max(worst, float(q.max()))
    return worst


def cosine(x, ref):
    x, ref = _as_matrix(x).flatten(), _as_matrix(ref).flatten()
    den = float(x.norm() * ref.norm())
    return float(x @ ref) / den if den > 0 else (1.0 if float(x.norm()) == float(ref.norm()) else 0.0)


def support(x, ref):
    """(rows non-zero where ref's row is exactly zero, worst relative L2 error over ref's non-zero rows, number of those)."""
    x, ref = _as_matrix(x), _as_matrix(ref)
    live = (ref != 0).any(1)
    stray = int((x[~live] != 0).any(1).sum())
    rel = (x[live] - ref[live]).norm(dim=1) / ref[live].norm(dim=1)
    return stray, float(rel.max()) if rel.numel() else 0.0, int(live.sum())


def measure_one(k, x, ref):
    m = {"block": block_error(x, ref)}
    if ref.numel() > 1:
        m["cos"] = cosine(x, ref)
    if k in SUPPORT_KEYS:
        m["stray_rows"], m["row_err"], m["live_rows"] = support(x, ref)
    return m


def measure(grads, ref):
    assert sorted(grads) == sorted(ref), (sorted(set(ref) - set(grads))[:5], sorted(set(grads) - set(ref))[:5])
    return {k: measure_one(k, grads[k], ref[k]) for k in ref}


def class_figures(m):
    """Per class: median and worst block error, lowest cosine, name of the worst tensor."""
    out = {}
    for c in CLASSES:
        ks = [k for k in m if tensor_class(k) == c]
        if not ks:
            continue
        worst = max(ks, key=lambda k: m[k]["block"])
        out[c] = {"n": len(ks), "median": float(np.median([m[k]["block"] for k in ks])), "worst": m[worst]["block"], "worst_name": worst,
                  "cos_lowest": min(m[k]["cos"] for k in ks if "cos" in m[k])}
    return out


def ratios(got, yard):
    """Per class, the distribution of got's block error over the yardstick's for the same tensor (the measured input of r)."""
    out = {}
    for c in CLASSES + ("scalar",):
        ks = [k for k in got if tensor_class(k) == c]
        if not ks:
            continue
        q = {k: got[k]["block"] / max(yard[k]["block"], 1e-12) for k in ks}
        worst = max(q, key=q.get)
        v = np.array(list(q.values()))
        out[c] = {"n": len(ks), "median": float(np.median(v)), "p90": float(np.percentile(v, 90)), "worst": q[worst], "worst_name": worst,
                  "worst_engine": got[worst]["block"], "worst_yardstick": yard[worst]["block"]}
    return out


def violations(got, yard, r, exceptions=None):
    """Every bound that `got` (measure() of the implementation) breaks against `yard` (measure() of the bf16 oracle), as strings.
    exceptions: {parameter name: extra block error allowed on top of the class-worst bound}, each explained where it is given;
    the bound against the tensor's own yardstick value takes no exception."""
    assert 0 < r <= R_MAX, r
    exceptions = exceptions or {}
    assert sorted(got) == sorted(yard)
    bad = []
    fg, fy = class_figures(got), class_figures(yard)
    for c in fy:
        if fg[c]["median"] > MEDIAN_FACTOR * fy[c]["median"] + MEDIAN_MARGIN:
            bad.append(f"{c}: median block error {fg[c]['median']:.4f} > {MEDIAN_FACTOR} x {fy[c]['median']:.4f} + {MEDIAN_MARGIN}")
    for k in got:
        c, g, y = tensor_class(k), got[k], yard[k]
        extra = exceptions.get(k, 0.0)
        # the worst the yardstick does in this tensor's class (logit_scale: the worse of itself and the token side, test_gpu_train.py)
        cls_worst = max(y["block"], fy["token"]["worst"]) if c == "scalar" else fy[c]["worst"]
        if g["block"] > cls_worst + WORST_MARGIN + extra:
            bad.append(f"{k}: block error {g['block']:.4f} > worst yardstick tensor of class {c} {cls_worst:.4f} + {WORST_MARGIN}")
        if g["block"] > r * y["block"] + OWN_MARGIN:
            bad.append(f"{k}: block error {g['block']:.4f} > {r:.3f} x its yardstick {y['block']:.4f} + {OWN_MARGIN}")
        if "cos" in g and c != "scalar" and g["cos"] < fy[c]["cos_lowest"] - COS_MARGIN:
            bad.append(f"{k}: cosine {g['cos']:.5f} < lowest yardstick cosine of class {c} {fy[c]['cos_lowest']:.5f} - {COS_MARGIN}")
        if k in SUPPORT_KEYS:
            if g["stray_rows"]:
                bad.append(f"{k}: {g['stray_rows']} rows that the reference leaves exactly zero are not zero")
            if g["row_err"] > y["row_err"] + WORST_MARGIN:                   # every row against the yardstick's worst row
                bad.append(f"{k}: worst touched row off by {g['row_err']:.4f} > the yardstick's worst row {y['row_err']:.4f} + {WORST_MARGIN}")
    return bad


def describe(tag, got, yard):
    fg, fy, q = class_figures(got), class_figures(yard), ratios(got, yard)
    lines = []
    for c in fy:
        lines.append(f"{tag} {c:5s} n {fg[c]['n']:3d} | block median {fg[c]['median']:.4f} (yardstick {fy[c]['median']:.4f}) worst {fg[c]['worst']:.4f} "
                     f"{fg[c]['worst_name']} (yardstick {fy[c]['worst']:.4f} {fy[c]['worst_name']}) | cosine {fg[c]['cos_lowest']:.5f} "
                     f"({fy[c]['cos_lowest']:.5f}) | got/yardstick median {q[c]['median']:.3f} p90 {q[c]['p90']:.3f} worst {q[c]['worst']:.3f} "
                     f"{q[c]['worst_name']} ({q[c]['worst_engine']:.4f} / {q[c]['worst_yardstick']:.4f})")
    if "logit_scale" in got:
        lines.append(f"{tag} logit_scale block {got['logit_scale']['block']:.4f} (yardstick {yard['logit_scale']['block']:.4f})")
    for k in SUPPORT_KEYS:
        if k in got:
            lines.append(f"{tag} {k}: {got[k]['live_rows']} touched rows, worst row {got[k]['row_err']:.4f} (yardstick {yard[k]['row_err']:.4f}), "
                         f"stray rows {got[k]['stray_rows']}")
    return "\n".join(lines)
