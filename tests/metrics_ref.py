"""numpy restatement of include/msclip_metrics.h (the counts of msclip_rank_counts), the cases that the CPU and GPU tests share, and
the scikit-learn oracle of the 11-point mAP (what tools/zero_shot.py:136-147 computes, in this project's words; the fixture tool and
the benchmark import it from here)."""
import re
import os

import numpy as np

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msclip_metrics.h")
with open(_HEADER) as _f:
    _TEXT = _f.read()
ROWS = int(re.search(r"^#define MSCLIP_RANK_ROWS (\d+)$", _TEXT, re.M).group(1))
STAGE = int(re.search(r"^#define MSCLIP_RANK_STAGE (\d+)$", _TEXT, re.M).group(1))
EDGE_N = (1, 2, ROWS - 1, ROWS, ROWS + 1, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 3)
SENTINEL = -77
KINDS = ("random", "equal", "seven levels", "signed zeros", "denormals", "infinities")


def counts(S, Y):
    """S fp32 [N, C], Y uint8 [N, C] -> ge_pos, ge_neg, gt_neg int32 [C, N], npos, nbad int32 [C]: the header's definitions, with
    numpy's (IEEE) comparisons on float32."""
    S, Y = np.asarray(S, dtype=np.float32), np.asarray(Y)
    N, C = S.shape
    ge_pos, ge_neg, gt_neg = (np.zeros((C, N), np.int32) for _ in range(3))
    npos, nbad = np.zeros(C, np.int32), np.zeros(C, np.int32)
    with np.errstate(invalid="ignore"):
        for c in range(C):
            s, pos = S[:, c], Y[:, c] != 0
            for i0 in range(0, N, 512):
                x = s[i0:i0 + 512, None]
                ge, gt = s[None, :] >= x, s[None, :] > x                 # [i, j]: S[j] >= S[i]
                ge_pos[c, i0:i0 + 512] = (ge & pos[None, :]).sum(1)
                ge_neg[c, i0:i0 + 512] = (ge & ~pos[None, :]).sum(1)
                gt_neg[c, i0:i0 + 512] = (gt & ~pos[None, :]).sum(1)
            npos[c], nbad[c] = pos.sum(), np.isnan(s).sum()
    return ge_pos, ge_neg, gt_neg, npos, nbad


def make_scores(kind, N, C, seed=0):
    """fp32 [N, C] scores of one of KINDS."""
    r = np.random.RandomState(seed)
    if kind == "random":
        S = r.randn(N, C) * 10
    elif kind == "equal":
        S = np.full((N, C), 0.375)
    elif kind == "seven levels":
        S = r.randint(0, 7, size=(N, C)) * 0.5 - 1.5
    elif kind == "signed zeros":                          # +0.0 and -0.0 are equal; one in eight is something else
        S = np.where(r.rand(N, C) < 0.125, r.randn(N, C), np.where(r.rand(N, C) < 0.5, 0.0, -0.0))
    elif kind == "denormals":                             # two distinct denormals, and zero: three levels that flushing would merge
        S = np.array([1e-45, 3e-45, 0.0], dtype=np.float32)[r.randint(0, 3, size=(N, C))]
    elif kind == "infinities":
        S = r.randn(N, C)
        u = r.rand(N, C)
        S[u < 0.2], S[u > 0.8] = np.inf, -np.inf
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(S, dtype=np.float32)


def make_labels(N, C, seed=0):
    """uint8 [N, C]: column 0 random over the bytes 0 / 1 / 255 / 7, column 1 (if any) all positive, column 2 all negative."""
    r = np.random.RandomState(seed + 1000)
    Y = np.where(r.rand(N, C) < 0.3, r.choice(np.array([1, 255, 7], np.uint8), size=(N, C)), 0).astype(np.uint8)
    if C > 1:
        Y[:, 1] = 1
    if C > 2:
        Y[:, 2] = 0
    return np.ascontiguousarray(Y)


def padded(a, ld, fill=0):
    """a [R, K] as the leading window of a [R, ld] matrix: (the wide matrix, its window)."""
    wide = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return wide, wide[:, :a.shape[1]]


# ---------------------------------------------------------------------------- the scikit-learn oracle
def sklearn_map11(labels, scores):
    """The 11-point average precision that tools/zero_shot.py:136-147 defines, computed from scikit-learn's curve: for each recall
    level of linspace(1, 0, 11), the best precision among the curve's points whose recall reaches the level; the eleven values
    added from level 1 down to level 0, over 11.  (The reference walks the curve once with a running maximum; recall never rises
    along scikit-learn's curve, so the points it has passed at a level are exactly those with recall >= level.)"""
    from sklearn.metrics import precision_recall_curve
    precision, recall, _ = precision_recall_curve(labels, scores)
    total = 0
    for level in np.linspace(1, 0, 11, endpoint=True).tolist():
        reached = precision[recall >= level]
        total += reached.max() if reached.size else 0
    return total / 11


def metric_cases():
    """[(name, scores fp32 [N], labels uint8 [N])]: random and tie-heavy columns, N <= 1100, and P = 10 (recalls on the deciles)."""
    r = np.random.RandomState(7)
    cases = []
    for k, N in enumerate((5, 17, 64, 257, 400, 1100)):
        for ties in (False, True):
            s = (r.randint(0, 6, size=N) * 0.25 if ties else r.randn(N)).astype(np.float32)
            y = (r.rand(N) < (0.1 + 0.1 * k)).astype(np.uint8)
            y[0], y[1] = 1, 0                                              # both classes occur
            cases.append((f"N{N}{' ties' if ties else ''}", s, y))
    for ties in (False, True):
        N = 300
        s = (r.randint(0, 9, size=N) * 0.5 if ties else r.randn(N)).astype(np.float32)
        y = np.zeros(N, np.uint8)
        y[r.permutation(N)[:10]] = 1
        cases.append((f"P10{' ties' if ties else ''}", s, y))
    return cases


def formulas(S, Y):
    """The per-column (ap11, auc or None where one class is absent) that msclip_amd.metrics gives on the restatement's counts."""
    from msclip_amd import metrics
    ge_pos, ge_neg, gt_neg, npos, nbad = counts(S, Y)
    ap = [metrics.ap11_from_counts(ge_pos[c], ge_neg[c], npos[c], nbad[c]) for c in range(S.shape[1])]
    auc = [metrics.auc_from_counts(ge_neg[c], gt_neg[c], Y[:, c] != 0, nbad[c]) if 0 < npos[c] < S.shape[0] else None
           for c in range(S.shape[1])]
    return ap, auc
