"""One evaluation of the linear probe's objective (linear_probe.ProbeObjective.value_and_grad) at ImageNet-1k size and at a
small-dataset size, over chunk_rows 4096 / 16384 / 65536, beside the same objective in plain torch fp32 ops (X @ W.T, log_softmax,
matmul: a vendor BLAS in fp32, another recipe -- reported, not gated), and the three kernels of a chunk on their own: achieved TB/s
of the row pass, TFLOP/s of the two GEMMs.  Warm-up, HIP event timing, 20 repetitions, median and spread.

    python tools/probes/linear_probe_bench.py [--reps 20] [--small-only] [--out profiles/linear_probe_bench.md]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import msclip_amd                                        # noqa: E402

msclip_amd.configure_runtime()
from msclip_amd import hip, linear_probe as LP           # noqa: E402

SHAPES = ((1_281_167, 512, 1000), (50_000, 512, 100))
CHUNKS = (4096, 16384, 65536)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_objective(X, y, P, l2, chunk):
    """The baseline: the same chunking, fp32 torch ops."""
    N, E = X.shape
    W, b = P[:, :E], P[:, E]
    dW, db, loss = torch.zeros_like(W), torch.zeros_like(b), torch.zeros((), device=X.device, dtype=torch.float64)
    for r0 in range(0, N, chunk):
        x, yy = X[r0:r0 + chunk], y[r0:r0 + chunk]
        lp = torch.log_softmax(x @ W.t() + b, 1)
        loss += -lp.gather(1, yy[:, None]).double().sum()
        G = lp.exp_()
        G.scatter_add_(1, yy[:, None], torch.full((len(yy), 1), -1.0, device=X.device))
        G /= N
        dW += G.t() @ x
        db += G.sum(0)
    return (loss / N + 0.5 * l2 * W.double().square().sum()).float(), torch.cat([dW + l2 * W, db[:, None]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip.require_gpu()
    lines = ["# Linear probe: one evaluation of the objective", "",
             f"{torch.cuda.get_device_name(0)}; HIP events, 3 warm-up + {a.reps} timed repetitions, median (min .. max) in ms.", ""]
    for N, E, C in (SHAPES[1:] if a.small_only else SHAPES):
        g = torch.Generator(device="cuda").manual_seed(0)
        X = torch.randn(N, E, device="cuda", generator=g)
        y = torch.randint(0, C, (N,), device="cuda", generator=g)
        P = 0.05 * torch.randn(C, E + 1, device="cuda", generator=g)
        lines += [f"## N = {N}, E = {E}, C = {C}", "", "| chunk_rows | device recipe | torch fp32 | ratio | loss (device / torch) |",
                  "|---|---|---|---|---|"]
        for chunk in CHUNKS:
            obj = LP.ProbeObjective(X, y.cpu(), C, 1e-4, chunk_rows=chunk)
            ours = timed(lambda: obj.value_and_grad(P), a.reps)
            base = timed(lambda: torch_objective(X, y, P, 1e-4, chunk), a.reps)
            l_dev, l_ref = float(obj.value_and_grad(P)[0]), float(torch_objective(X, y, P, 1e-4, chunk)[0])
            lines.append(f"| {chunk} | {ours[0]:.2f} ({ours[1]:.2f} .. {ours[2]:.2f}) | {base[0]:.2f} ({base[1]:.2f} .. {base[2]:.2f}) | "
                         f"{base[0] / ours[0]:.2f}x | {l_dev:.6f} / {l_ref:.6f} |")
            if chunk == 16384:                       # the kernels of one full chunk on their own
                R, Cpad, Ep = obj.chunk, obj.Cpad, obj.Ep
                rows = obj.X3[:R]
                obj.fw.set_params(P)
                S = obj.fw.logits(rows)
                nwg = (R + hip.PROBE_ROWS - 1) // hip.PROBE_ROWS
                t_g = timed(lambda: obj.fw.logits(rows), a.reps)
                t_r = timed(lambda: hip.probe_ce_rows(S, obj.fw.bias, obj.y32[:R], C, 1.0 / N, G_hi=obj.Gh[:R], G_lo=obj.Gl[:R],
                                                      loss_part=obj.loss_part[:nwg], colsum_part=obj.col_part[:nwg],
                                                      bad_part=obj.bad_part[:nwg]), a.reps)
                dWa = torch.empty(Cpad, 2 * Ep, device="cuda")
                dWb = torch.empty(Cpad, Ep, device="cuda")

                def tn():
                    obj._tn_add(obj.Gh[:R], rows[:, Ep:], R, dWa, True)
                    obj._tn_add(obj.Gl[:R], rows[:, :Ep], R, dWb, True)
                t_t = timed(tn, a.reps)
                fl = 2.0 * R * Cpad * 3 * Ep
                kern = [f"chunk of {R} rows, Cpad {Cpad}: logits GEMM {t_g[0]:.3f} ms = {fl / t_g[0] / 1e9:.0f} TFLOP/s; "
                        f"row pass {t_r[0]:.3f} ms = {R * Cpad * 8 / t_r[0] / 1e9:.2f} TB/s of its R Cpad (4 + 2 + 2) bytes; "
                        f"weight-gradient GEMMs + folds {t_t[0]:.3f} ms = {fl / t_t[0] / 1e9:.0f} TFLOP/s"]
            del obj
        lines += [""] + kern + [""]
        del X, y, P
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
