"""The linear probe's objective restated in fp64 torch, for the tests (no GPU):

    f(P) = (1/N) sum_i ( logsumexp_c(x_i . W_c + b_c) - (x_i . W_{y_i} + b_{y_i}) ) + (l2/2) ||W||_F^2,   P = [W | b] of [C, E + 1]

and an EMULATION of the device recipe (msclip_amd/linear_probe.py): bf16 hi/lo splits of X, W and G, the three-term products
hi.hi + hi.lo + lo.hi, every sum in fp64.  The emulation's distance from the fp64 values is what the recipe itself costs; the GPU
tests bound the device's distance by a multiple of it."""
import torch

F64 = torch.float64


def split(t):
    """fp32 tensor -> (hi, lo) as fp64 tensors holding bf16 values: hi = bf16(t), lo = bf16(t - float(hi))."""
    t = t.float()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.to(F64), lo.to(F64)


def objective(P, X, y, l2):
    """-> (loss, grad [C, E + 1]) in fp64, closed form."""
    P, X = P.to(F64), X.to(F64)
    N, E = X.shape
    W, b = P[:, :E], P[:, E]
    S = X @ W.t() + b
    lse = torch.logsumexp(S, 1)
    loss = (lse - S[torch.arange(N), y]).mean() + 0.5 * l2 * (W * W).sum()
    G = torch.softmax(S, 1)
    G[torch.arange(N), y] -= 1.0
    G /= N
    return loss, torch.cat([G.t() @ X + l2 * W, G.sum(0)[:, None]], 1)


def objective_autograd(P, X, y, l2):
    """The same through autograd of the loss as written (the check of `objective`)."""
    P = P.to(F64).clone().requires_grad_(True)
    X = X.to(F64)
    E = X.shape[1]
    S = X @ P[:, :E].t() + P[:, E]
    loss = torch.nn.functional.cross_entropy(S, y) + 0.5 * l2 * P[:, :E].square().sum()
    loss.backward()
    return loss.detach(), P.grad


def emulate(P, X, y, l2):
    """The device recipe with exact accumulation: logits from the split operands (the lo.lo term dropped), the bias and the
    statistics from those logits, G = (softmax - onehot) / N rounded to fp32 and split, dW from the three terms of G and X, db from
    the fp32 G.  -> (loss, grad) in fp64."""
    P, X = P.float(), X.float()
    N, E = X.shape
    W, b = P[:, :E], P[:, E].to(F64)
    xh, xl = split(X)
    wh, wl = split(W)
    S = (xh @ wh.t() + xh @ wl.t() + xl @ wh.t()).float().to(F64) + b          # the GEMM's output is fp32
    lse = torch.logsumexp(S, 1)
    loss = (lse - S[torch.arange(N), y]).mean() + 0.5 * l2 * (W.to(F64) ** 2).sum()
    G = torch.softmax(S, 1)
    G[torch.arange(N), y] -= 1.0
    G = (G / N).float()
    gh, gl = split(G)
    dW = gh.t() @ xh + gh.t() @ xl + gl.t() @ xh
    return loss, torch.cat([dW + l2 * W.to(F64), G.to(F64).sum(0)[:, None]], 1)


def centre(P):
    """P with the mean bias removed: the objective does not see a common shift of b."""
    P = P.to(F64).clone()
    P[:, -1] -= P[:, -1].mean()
    return P


def rel_distance(P, Q):
    """|| centre(P) - centre(Q) || / || centre(Q) ||."""
    P, Q = centre(P), centre(Q)
    return float((P - Q).norm() / Q.norm())


def fit_lbfgs(X, y, C, l2, value_and_grad=objective, max_iter=1000, dtype=F64):
    """torch.optim.LBFGS (strong Wolfe, lr 1, history 10) on the CPU, driven by `value_and_grad` -- the driver linear_probe.fit
    uses, on the reference objective (or on `emulate`)."""
    P = torch.zeros(C, X.shape[1] + 1, dtype=dtype, requires_grad=True)
    opt = torch.optim.LBFGS([P], lr=1, max_iter=max_iter, history_size=10, tolerance_grad=1e-7 if dtype != F64 else 1e-12,
                            tolerance_change=1e-12 if dtype != F64 else 1e-16, line_search_fn="strong_wolfe")

    def closure():
        loss, g = value_and_grad(P.detach(), X, y, l2)
        P.grad = g.to(dtype)
        return loss
    opt.step(closure)
    return P.detach()
