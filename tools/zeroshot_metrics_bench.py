"""Time of the zero-shot ranking metrics on the device (msclip_rank_counts behind msclip_amd.metrics.average_precision_11 / roc_auc)
next to the reference's path on the same logits: copy them to the host and hand every column to scikit-learn (tools/zero_shot.py:
280-300).

    python tools/zeroshot_metrics_bench.py [--shapes 4952x20,50000x80] [--reps 20] [--out FILE.json]

Per shape: the call (HIP events around msclip_rank_counts: the launch path and the kernel, median of --reps after 3 warm-up calls, outputs preallocated),
the driver end to end (kernel, one copy of the integers to the host, the float64 formulas; host clock around a call that ends with
the values on the host), and scikit-learn's path (device-to-host copy of the logits included; skipped where scikit-learn is
absent).  Prints one JSON record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msclip_amd                                                   # noqa: E402

msclip_amd.configure_runtime()
import numpy as np                                                  # noqa: E402
import torch                                                        # noqa: E402


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def one_shape(N, C, reps):
    from msclip_amd import metrics, metrics_hip
    r = np.random.RandomState(N + C)
    S = torch.from_numpy((r.randn(N, C) * 3).astype(np.float32)).cuda()          # logits-like: no ties to speak of
    Y = torch.from_numpy((r.rand(N, C) < 0.08).astype(np.uint8))
    Y[0], Y[1] = 1, 0
    Yd = Y.cuda()
    out = metrics_hip.rank_counts(S, Yd)
    torch.cuda.synchronize()
    ms = []
    for k in range(3 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        metrics_hip.rank_counts(S, Yd, out=out)
        e1.record()
        e1.synchronize()
        if k >= 3:
            ms.append(e0.elapsed_time(e1))
    rec = dict(N=N, C=C, pairs=N * N * C, launches=len(metrics_hip.class_chunks(N, C)), call_ms=median(ms), call_ms_min=min(ms),
               call_ms_max=max(ms), pairs_per_s=N * N * C / (median(ms) * 1e-3))
    drv, auc = [], []
    for k in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mean, per = metrics.average_precision_11(S, Yd)
        drv.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        a = metrics.roc_auc(S, Y[:, 0], column=min(1, C - 1))
        auc.append((time.perf_counter() - t0) * 1e3)
    rec.update(map11_driver_ms=median(drv[2:]), roc_auc_driver_ms=median(auc[2:]), map11=mean, roc_auc=a)
    try:
        from sklearn.metrics import roc_auc_score
        from metrics_ref import sklearn_map11
    except ImportError:
        rec["sklearn"] = None
        return rec
    sk, ska = [], []
    for k in range(1 + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logits, y = S.cpu(), Y
        total = 0
        for c in range(C):
            total += sklearn_map11(y[:, c], logits[:, c])
        sk.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        logits = S.cpu()
        b = roc_auc_score(Y[:, 0], logits[:, min(1, C - 1)])
        ska.append((time.perf_counter() - t0) * 1e3)
    import sklearn
    rec.update(sklearn=sklearn.__version__, sklearn_map11_ms=median(sk[1:]), sklearn_roc_auc_ms=median(ska[1:]),
               map11_diff=abs(total / C - mean), roc_auc_diff=abs(a - b))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4952x20,50000x80")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one_shape(*(int(v) for v in s.split("x")), a.reps) for s in a.shapes.split(",")]
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), reps=a.reps, shapes=recs))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
