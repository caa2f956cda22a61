"""The zero-shot metrics besides top-1 accuracy (reference tools/zero_shot.py:136-147, 280-300: TEST.METRIC 11point_mAP, roc_auc and
mean-per-class, which the reference computes with scikit-learn on logits copied to the host).

Here the logits stay on the device.  msclip_rank_counts (include/msclip_metrics.h) turns a column of scores and labels into exact
integers: for every sample, the positives and negatives that score at least as high.  The formulas below are applied to those
integers on the host in float64; they need no GPU (tests/test_metrics_cpu.py runs them on a numpy restatement of the counts).

* ap11_from_counts   the reference's mAP_11points of one class, quirks included
* auc_from_counts    roc_auc_score of one column: Mann-Whitney's statistic with ties counted half
* mean_per_class     balanced_accuracy_score: the mean over the classes that occur of each class's recall
* average_precision_11, roc_auc, predict_rows: the device drivers
"""
import numpy as np
import torch

RECALL_THRESHOLDS = np.linspace(1, 0, 11, endpoint=True).tolist()          # zero_shot.py:138


def _check_column(nbad, what):
    if int(nbad) != 0:
        raise ValueError(f"{what}: {int(nbad)} scores are not a number")      # scikit-learn: "Input contains NaN."


def ap11_from_counts(ge_pos, ge_neg, npos, nbad=0):
    """11-point average precision of one class from its counts (int arrays [N]; npos: the number of positives).

    The curve has one point per sample: precision TP / (TP + FP) and recall TP / P at that sample's score as the threshold, TP =
    ge_pos, FP = ge_neg (precision_recall_curve keeps one point per distinct score: the same set).  For each of the eleven recall
    levels 1.0, 0.9 ... 0.0 the term is the largest precision among the points whose recall reaches the level; the level 0 always
    gives 1.0, because precision_recall_curve appends the point (precision 1, recall 0).  The terms are added in that order and
    divided by 11.  Without a positive scikit-learn sets every recall to 1 (and every precision is 0): 1 / 11."""
    _check_column(nbad, "ap11_from_counts")
    tp, fp = np.asarray(ge_pos, dtype=np.float64), np.asarray(ge_neg, dtype=np.float64)
    P = int(npos)
    precision = tp / (tp + fp)
    recall = tp / float(P) if P > 0 else np.ones_like(tp)
    total = 0
    for level in RECALL_THRESHOLDS[:-1]:
        reach = recall >= level
        total += float(precision[reach].max()) if reach.any() else 0
    total += 1.0
    return total / 11


def map11_percent(per_class):
    """The per-class values added in class order, times 100, over the number of classes (zero_shot.py:283-286)."""
    total = 0
    for v in per_class:
        total += v
    return total * 100 / len(per_class)


def auc_from_counts(ge_neg, gt_neg, positive, nbad=0):
    """Area under the ROC curve of one column from its counts (int arrays [N]; positive: bool [N]).  Each positive scores one for
    every negative strictly below it and a half for every negative it ties with: sum / (P * Nneg).  The sum is an integer (in
    halves), so the result is one division away from exact."""
    _check_column(nbad, "auc_from_counts")
    pos = np.asarray(positive).astype(bool)
    N, P = pos.size, int(pos.sum())
    if P == 0 or P == N:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    nneg = N - P
    ge, gt = np.asarray(ge_neg, dtype=np.int64)[pos], np.asarray(gt_neg, dtype=np.int64)[pos]
    halves = int((2 * (nneg - ge) + (ge - gt)).sum())
    return halves / (2.0 * P * nneg)


def mean_per_class(pred, y, num_classes):
    """balanced_accuracy_score in [0, 1]: pred and y integer arrays or tensors [N] (a device tensor is copied to the host once).
    A class that no label names does not count."""
    from .linear_probe import score_counts
    pred = (pred.detach().cpu() if torch.is_tensor(pred) else torch.as_tensor(np.asarray(pred))).long()
    y = y.detach().cpu() if torch.is_tensor(y) else np.asarray(y)
    return score_counts(pred, torch.zeros_like(pred), y, num_classes, "mean_per_class")["top1"] / 100.0


# ---------------------------------------------------------------------------------------------------------------------
# device drivers
# ---------------------------------------------------------------------------------------------------------------------
def _labels_u8(Y, like):
    Y = torch.as_tensor(Y)
    return (Y != 0).to(device=like.device, dtype=torch.uint8)


def average_precision_11(S, Y):
    """S fp32 [N, C] logits on the device, Y [N, C] multi-hot labels (any integer / bool tensor or array; not 0 = positive)
    -> (the mean over the classes in [0, 1], the per-class list).  One kernel pass, one copy of the integers to the host."""
    from . import metrics_hip
    Y8 = _labels_u8(Y, S)
    if Y8.dim() != 2 or tuple(Y8.shape) != tuple(S.shape):
        raise ValueError(f"average_precision_11: labels {list(Y8.shape)} for scores {list(S.shape)}")
    ge_pos, ge_neg, _, npos, nbad = metrics_hip.rank_counts(S, Y8, want_gt=False)
    ge_pos, ge_neg, npos, nbad = (t.cpu().numpy() for t in (ge_pos, ge_neg, npos, nbad))
    per = [ap11_from_counts(ge_pos[c], ge_neg[c], npos[c], nbad[c]) for c in range(S.shape[1])]
    return map11_percent(per) / 100.0, per


def roc_auc(S, y, column=1):
    """S fp32 [N, C] logits on the device, y [N] binary labels -> the area under the ROC curve of S[:, column] (zero_shot.py:299)."""
    from . import metrics_hip
    if S.dim() != 2 or not 0 <= column < S.shape[1]:
        raise ValueError(f"roc_auc: column {column} of scores {list(S.shape)}")
    y = torch.as_tensor(y).reshape(-1)
    if y.numel() != S.shape[0]:
        raise ValueError(f"roc_auc: {y.numel()} labels for {S.shape[0]} scores")
    if bool(((y != 0) & (y != 1)).any()):
        raise ValueError("roc_auc: labels must be 0 or 1")
    Y8 = _labels_u8(y, S).reshape(-1, 1)
    _, ge_neg, gt_neg, _, nbad = metrics_hip.rank_counts(S[:, column:column + 1], Y8)
    ge_neg, gt_neg, nbad = (t.cpu().numpy() for t in (ge_neg, gt_neg, nbad))
    return auc_from_counts(ge_neg[0], gt_neg[0], (y != 0).cpu().numpy(), nbad[0])


def predict_rows(S, y32, pred, rank=None):
    """Argmax (lowest index on ties, as the reference's host argmax) of every row of the fp32 device block S [R, C] into pred (int32
    [R] device) and, where asked for, the label's rank into rank: msclip_probe_ce_rows in its predict-only form."""
    from . import hip
    hip.probe_ce_rows(S, None, y32, S.shape[1], 1.0, pred=pred, rank=rank)
