"""Writes tests/golden/linear_probe_fixture.npz: two small softmax-regression problems solved by scikit-learn, the yardstick of
msclip_amd/linear_probe.py's fit (the GPU tests read the file and never import sklearn).

    python tools/make_golden_probe.py [--seed 0] [--out tests/golden/linear_probe_fixture.npz]

The data: C = 7 Gaussian class clusters in E = 64 dimensions (centres sep * N(0, 1), unit noise), N = 600 training rows and a 300-row
held-out set from the same clusters, as fp32.  `sep` is the first value of a fixed list at which the fp64 classifier's held-out top-1
lies in [0.6, 0.9] for both penalties -- a fixture on which every held-out row is right would test nothing about prediction.  The two
problems share the data and differ in l2 in {1e-3, 1e-2}; each is fitted with
    LogisticRegression(C=1 / (l2 * N), tol=1e-10, max_iter=5000)         (lbfgs, multinomial, fp64)
which minimises N times the objective of linear_probe.py.  Stored: X, y, Xval, yval, l2 [2], P [2, C, E + 1] = (coef_ | intercept_),
the fp64 held-out logits [2, 300, C], sep, seed.  The tool refuses a fixture in which more than 1 % of the held-out rows have an
fp64 top-2 margin below 1e-3 * max|logit| (tests/test_gpu_linear_probe.py leaves such rows out): try another seed then."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NVAL, E, C = 600, 300, 64, 7
L2 = (1e-3, 1e-2)
SEPS = (0.35, 0.3, 0.25, 0.2, 0.17, 0.15, 0.12, 0.1)


def make_data(seed, sep):
    rng = np.random.default_rng(seed)
    centres = sep * rng.standard_normal((C, E))
    y, yval = np.arange(N) % C, np.arange(NVAL) % C
    rng.shuffle(y)
    rng.shuffle(yval)
    X = (centres[y] + rng.standard_normal((N, E))).astype(np.float32)
    Xval = (centres[yval] + rng.standard_normal((NVAL, E))).astype(np.float32)
    return X, y.astype(np.int64), Xval, yval.astype(np.int64)


def solve(X, y, l2):
    from sklearn.linear_model import LogisticRegression
    clf = LogisticRegression(C=1.0 / (l2 * len(X)), tol=1e-10, max_iter=5000).fit(X.astype(np.float64), y)
    return np.concatenate([clf.coef_, clf.intercept_[:, None]], 1)


def low_margin_share(S):
    top = np.sort(S, 1)
    return float(np.mean(top[:, -1] - top[:, -2] < 1e-3 * np.abs(S).max()))


def build(seed):
    for sep in SEPS:
        X, y, Xval, yval = make_data(seed, sep)
        P = np.stack([solve(X, y, l2) for l2 in L2])
        S = np.stack([Xval.astype(np.float64) @ p[:, :E].T + p[:, E] for p in P])
        acc = [float(np.mean(s.argmax(1) == yval)) for s in S]
        print(f"sep {sep}: held-out top-1 {acc}, rows under the margin {[low_margin_share(s) for s in S]}")
        if all(0.6 <= a <= 0.9 for a in acc):
            if max(low_margin_share(s) for s in S) > 0.01:
                raise SystemExit("more than 1 % of the held-out rows under the margin: use another --seed")
            return dict(X=X, y=y, Xval=Xval, yval=yval, l2=np.array(L2), P=P, val_logits=S, sep=np.array(sep), seed=np.array(seed))
    raise SystemExit("no separation of the list gives a held-out top-1 in [0.6, 0.9]")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "linear_probe_fixture.npz"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    np.savez(a.out, **build(a.seed))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
