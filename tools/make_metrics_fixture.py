"""Writes tests/golden/zeroshot_metrics_fixture.npz: the score / label columns of tests/metrics_ref.metric_cases with the values the
reference's code gives on them through scikit-learn (the 11-point mAP over precision_recall_curve, roc_auc_score), and one multi-class
case with balanced_accuracy_score of its argmax.  The fixture carries the comparison to machines without scikit-learn.

    python tools/make_metrics_fixture.py          # needs scikit-learn (written with 1.7.2)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_ref as R                                 # noqa: E402


def multiclass_case():
    """Logits fp32 [240, 7] with ties (the argmax takes the lowest index) and labels in which class 5 never occurs."""
    r = np.random.RandomState(11)
    logits = (r.randint(0, 12, size=(240, 7)) * 0.5).astype(np.float32)
    y = r.choice(np.array([0, 1, 2, 3, 4, 6]), size=240)
    return logits, y.astype(np.int64)


def main():
    import sklearn
    from sklearn.metrics import balanced_accuracy_score, roc_auc_score
    out = {"sklearn_version": np.array(sklearn.__version__)}
    cases = R.metric_cases()
    out["names"] = np.array([name for name, _, _ in cases])
    for k, (_, s, y) in enumerate(cases):
        out[f"s{k}"], out[f"y{k}"] = s, y
    out["ap11"] = np.array([R.sklearn_map11(y, s) for _, s, y in cases], dtype=np.float64)
    out["auc"] = np.array([roc_auc_score(y, s) for _, s, y in cases], dtype=np.float64)
    logits, y = multiclass_case()
    out["mc_logits"], out["mc_labels"] = logits, y
    out["mc_balanced"] = np.array(balanced_accuracy_score(y, logits.argmax(-1)), dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "zeroshot_metrics_fixture.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} columns, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
