"""Linear-probe evaluation: a softmax classifier fitted on frozen image features, every pass over the features on the device.

The objective.  Features X [N, E] fp32, labels y in [0, C), parameters P = [W | b] of shape [C, E + 1] fp32:

    f(P) = (1/N) * sum_i ( logsumexp_c(x_i . W_c + b_c) - (x_i . W_{y_i} + b_{y_i}) )  +  (l2/2) * ||W||_F^2      (b is not penalised)

This is scikit-learn's multinomial LogisticRegression(C=Csk) with l2 = 1 / (Csk * N) (l2_from_csk / csk_from_l2).  CLIP's
published protocol -- Csk = 0.316, L-BFGS, max_iter = 1000, on the un-normalised projected image features, no augmentation --
is the default here: features="proj" is encode_image(norm=False), normalize=True is an option.  The reference ships no
linear-probe code, so the protocol is parity-unpinned by construction (DESIGN.md "Linear probe").  For l2 > 0 the objective is
strictly convex in W and convex in b up to a common shift of all biases.

One evaluation (ProbeObjective.value_and_grad), in row chunks of `chunk_rows` so that no [N, C] matrix of the whole set ever exists:

    once per fit     X -> bf16 (hi | hi | lo) [N, 3 E]                       msclip_split_bf16 (include/msclip_ext5.h)
    per evaluation   W -> bf16 (hi | lo | hi) [Cpad, 3 E]                    msclip_split_bf16
    per chunk        S = X W^T, fp32 [R, Cpad], K = 3 E (the three products hi.hi + hi.lo + lo.hi of the training head)     msclip_gemm
                     lse, G = (softmax - onehot) / N as bf16 hi + lo, loss and bias-gradient partials     msclip_probe_ce_rows
                     dW += G_hi^T (X_hi | X_lo) and G_lo^T X_hi (token-major, no transposes)              msclip_gemm_splitk_tn
                     db += column sums of the fp32 G                                                      msclip_colsum
    once             loss = (sum of the partials, in double) / N                                          msclip_probe_loss_fold

Chunk partials of dW and db are added in chunk order: a given chunk_rows gives the same bits every time.  Padding, because of the
GEMMs' shape rules: the class count is padded to Cpad = a multiple of 16 with zero rows of W (their logits are never read as
classes, their G columns are written as zero), E to a multiple of 64 with zero columns, and the split features carry one zero row
behind the last one.  torch's part: L-BFGS's two-loop recursion and line search on the [C, E + 1] vectors (2 MB at 1000 x 512), the
l2 term of those vectors, and the host logic below.
"""
import ctypes
import hashlib
import os
import time

import numpy as np
import torch

from . import hip, zeroshot

F32, BF16 = torch.float32, torch.bfloat16
FEATURES = ("proj",)
METRICS = ("accuracy", "mean_per_class")


def l2_from_csk(csk, n):
    """scikit-learn's C (an inverse penalty on the SUM of the losses) -> l2 of the objective above (a penalty beside their MEAN)."""
    return 1.0 / (float(csk) * int(n))


def csk_from_l2(l2, n):
    return 1.0 / (float(l2) * int(n))


def _round_up(n, m):
    return (n + m - 1) // m * m


def _split3(X, order, extra_rows=0):
    """fp32 [M, E] (device) -> bf16 [M + extra_rows, 3 Ep] with Ep = E rounded up to 64 and zero padding: order "hhl" = (hi | hi | lo),
    the features' side of the K = 3 E contraction; "hlh" = (hi | lo | hi), the weights' side."""
    M, E = X.shape
    Ep = _round_up(E, 64)
    if Ep != E:
        X = torch.nn.functional.pad(X, (0, Ep - E))
    out = torch.empty(M + extra_rows, 3 * Ep, dtype=BF16, device=X.device)
    if extra_rows:
        out[M:].zero_()
    if order == "hhl":
        hip.split_bf16(X, out[:M, Ep:])
        out[:M, :Ep].copy_(out[:M, Ep:2 * Ep])
    else:
        hip.split_bf16(X, out[:M, :2 * Ep])
        out[:M, 2 * Ep:].copy_(out[:M, :Ep])
    return out


def _labels32(y, num_classes, device):
    """-> int32 device labels.  Labels that are host-visible are checked here; device labels are clamped by the kernel, which
    counts them (ProbeObjective.check_labels)."""
    y = torch.as_tensor(y)
    if not y.is_cuda and y.numel() and (int(y.min()) < 0 or int(y.max()) >= num_classes):
        raise ValueError(f"labels must lie in [0, {num_classes}): got [{int(y.min())}, {int(y.max())}]")
    return y.to(device=device, dtype=torch.int32).contiguous()


class _Logits:
    """The forward half shared by the objective and by prediction: P -> the split weights, a chunk of split features -> S."""

    def __init__(self, num_classes, E, chunk_rows, device):
        self.C, self.E, self.Ep, self.Cpad = int(num_classes), int(E), _round_up(E, 64), _round_up(num_classes, 16)
        self.chunk, self.dev = int(chunk_rows), device
        if self.C < 2 or self.chunk <= 0:
            raise ValueError("linear probe: num_classes >= 2 and chunk_rows >= 1")
        self.Wp = torch.zeros(self.Cpad, self.E, dtype=F32, device=device)
        self.S = None

    def set_params(self, P):
        if tuple(P.shape) != (self.C, self.E + 1) or P.dtype != F32 or P.device != self.dev:
            raise ValueError(f"P must be fp32 [{self.C}, {self.E + 1}] on {self.dev}, got {P.dtype} {tuple(P.shape)} on {P.device}")
        self.Wp[:self.C].copy_(P[:, :self.E])
        self.W3 = _split3(self.Wp, "hlh")
        self.bias = P[:, self.E].contiguous()

    def logits(self, X3rows):
        R = X3rows.shape[0]
        if self.S is None or self.S.shape[0] < R:
            self.S = torch.empty(R, self.Cpad, dtype=F32, device=self.dev)      # (the first chunk is the largest)
        S = self.S[:R]
        hip.gemm(X3rows, self.W3, S)
        return S


class ProbeObjective:
    """f(P) of the module docstring and its gradient for one feature set.  X: fp32 device tensor [N, E], split once (the fp32
    copy is not kept); y: labels in [0, num_classes); l2 may be reassigned between evaluations (sweep does).  `evals` counts the
    evaluations."""

    def __init__(self, X, y, num_classes, l2, chunk_rows=65536):
        hip.require_gpu()
        if not (torch.is_tensor(X) and X.is_cuda and X.dtype == F32 and X.dim() == 2 and X.shape[0] > 0):
            raise ValueError("ProbeObjective: X must be a non-empty fp32 [N, E] tensor on the GPU (there is no CPU path)")
        self.dev = X.device
        self.N, self.E = X.shape
        self.l2, self.evals = float(l2), 0
        with torch.cuda.device(self.dev):
            self.fw = _Logits(num_classes, self.E, chunk_rows, self.dev)
            self.C, self.Cpad, self.Ep, self.chunk = self.fw.C, self.fw.Cpad, self.fw.Ep, min(self.fw.chunk, self.N)
            self.y32 = _labels32(y, self.C, self.dev)
            if self.y32.numel() != self.N:
                raise ValueError(f"{self.y32.numel()} labels for {self.N} rows")
            # one zero row behind the last: the token-major GEMM's address range over the (hi | lo) column window ends Ep columns
            # behind the window's last row
            self.X3 = _split3(X.contiguous(), "hhl", extra_rows=1)
            R, wg = self.chunk, hip.PROBE_ROWS
            self.n_wg = sum((min(R, self.N - r0) + wg - 1) // wg for r0 in range(0, self.N, R))
            self.Gh = torch.empty(R, self.Cpad, dtype=BF16, device=self.dev)
            self.Gl = torch.empty(R, self.Cpad, dtype=BF16, device=self.dev)
            self.loss_part = torch.empty(self.n_wg, dtype=torch.float64, device=self.dev)
            self.bad_part = torch.empty(self.n_wg, dtype=torch.int32, device=self.dev)
            self.col_part = torch.empty((R + wg - 1) // wg, self.Cpad, dtype=F32, device=self.dev)
            tiles = ((self.Cpad + 255) // 256) * ((2 * self.Ep + 255) // 256)
            self.slices = max(1, min(256 // tiles, R // 2048))                  # token ranges of the weight-gradient GEMM, at most
            self.tn_part = torch.empty(self.slices * self.Cpad * 2 * self.Ep, dtype=F32, device=self.dev)
            self.loss64 = torch.zeros(1, dtype=torch.float64, device=self.dev)

    def _tn_add(self, G, x, T, acc, first):
        """acc [Cpad, x's width] (+)= G[:T]^T x[:T]: msclip_gemm_splitk_tn into slice partials, folded into acc by msclip_colsum."""
        Mo, No = G.shape[1], x.shape[1]
        slices = max(1, min(self.slices, T // 2048))      # (every slice holds rows: gradgemm's rule, from the chunk's own row count)
        part = self.tn_part[:slices * Mo * No].view(slices, Mo * No)                 # slice s lies Mo * No floats behind slice s - 1
        d = hip.GemmDesc()
        d.X, d.W, d.zero, d.out = G.data_ptr(), x.data_ptr(), hip.zero_page(self.dev).data_ptr(), part.data_ptr()
        d.M, d.N, d.K, d.ldx, d.ldw, d.ldo = Mo, No, T, G.stride(0), x.stride(0), No
        d.out_kind, d.alpha, d.rpg = 1, 1.0, hip.INT_MAX
        hip._check(hip.lib().msclip_gemm_splitk_tn(ctypes.byref(d), slices, hip._stream()), "msclip_gemm_splitk_tn")
        hip.colsum(part, out=acc.view(-1), accumulate=not first)

    @hip.off_default_stream
    def value_and_grad(self, P, loss64=False):
        """-> (loss [] , grad [C, E + 1]), fp32 device tensors; loss64=True returns the loss as the float64 scalar it is folded in
        (fit hands that one to the line search)."""
        with torch.cuda.device(self.dev), torch.no_grad():
            fw, C, E, Ep, Cpad = self.fw, self.C, self.E, self.Ep, self.Cpad
            fw.set_params(P.detach())
            dWa = torch.empty(Cpad, 2 * Ep, dtype=F32, device=self.dev)
            dWb = torch.empty(Cpad, Ep, dtype=F32, device=self.dev)
            db = torch.empty(Cpad, dtype=F32, device=self.dev)
            w, wg0 = 1.0 / self.N, 0
            for k, r0 in enumerate(range(0, self.N, self.chunk)):
                R = min(self.chunk, self.N - r0)
                nwg = (R + hip.PROBE_ROWS - 1) // hip.PROBE_ROWS
                rows = self.X3[r0:r0 + R]
                S = fw.logits(rows)
                hip.probe_ce_rows(S, fw.bias, self.y32[r0:r0 + R], C, w, G_hi=self.Gh[:R], G_lo=self.Gl[:R],
                                  loss_part=self.loss_part[wg0:wg0 + nwg], colsum_part=self.col_part[:nwg],
                                  bad_part=self.bad_part[wg0:wg0 + nwg])
                hip.colsum(self.col_part[:nwg], out=db, accumulate=k > 0)
                self._tn_add(self.Gh[:R], rows[:, Ep:], R, dWa, k == 0)        # G_hi^T (X_hi | X_lo)
                self._tn_add(self.Gl[:R], rows[:, :Ep], R, dWb, k == 0)        # G_lo^T X_hi
                wg0 += nwg
            hip.probe_loss_fold(self.loss_part, self.n_wg, self.N, self.loss64)
            W = P.detach()[:, :E]
            grad = torch.empty(C, E + 1, dtype=F32, device=self.dev)
            grad[:, :E] = (dWa[:C, :E] + dWa[:C, Ep:Ep + E]) + dWb[:C, :E] + self.l2 * W
            grad[:, E] = db[:C]
            loss = self.loss64[0] + 0.5 * self.l2 * W.double().square().sum()
            self.evals += 1
            return (loss if loss64 else loss.float()), grad

    @hip.off_default_stream
    def predict(self, P, X2, y2=None):
        """-> (pred int32 [M], rank int32 [M] or None without labels) for another fp32 feature matrix X2 [M, E]."""
        return _predict(self.fw, P, X2, y2)

    def check_labels(self):
        """Raises if an evaluation met a label outside [0, C) (device labels: the kernel clamps and counts them)."""
        if self.evals and int(self.bad_part.sum()):
            raise ValueError(f"{int(self.bad_part.sum())} labels outside [0, {self.C}) in the training set")


def _predict(fw, P, X, y=None):
    with torch.cuda.device(fw.dev), torch.no_grad():
        if not (X.is_cuda and X.dtype == F32 and X.dim() == 2 and X.shape[1] == fw.E):
            raise ValueError(f"features must be fp32 [M, {fw.E}] on the GPU")
        M = X.shape[0]
        fw.set_params(P.detach())
        pred = torch.empty(M, dtype=torch.int32, device=fw.dev)
        y32 = _labels32(y, fw.C, fw.dev) if y is not None else None
        rank = torch.empty(M, dtype=torch.int32, device=fw.dev) if y is not None else None
        for r0 in range(0, M, fw.chunk):
            R = min(fw.chunk, M - r0)
            S = fw.logits(_split3(X[r0:r0 + R].contiguous(), "hhl"))
            hip.probe_ce_rows(S, fw.bias, y32[r0:r0 + R] if y is not None else None, fw.C, 1.0 / M, pred=pred[r0:r0 + R],
                              rank=rank[r0:r0 + R] if y is not None else None)
        return pred, rank


def predict(P, X, y=None, chunk_rows=65536):
    """-> (pred, rank): the argmax class of every row of X (lowest index on ties) and, with labels, the number of classes scoring
    strictly higher than the label (top-k hit = rank < k)."""
    hip.require_gpu()
    return _predict(_Logits(P.shape[0], P.shape[1] - 1, chunk_rows, X.device), P, X, y)


def fit(X, y, num_classes, l2, max_iter=1000, history=10, tol_grad=1e-7, tol_change=1e-12, init=None, chunk_rows=65536,
        objective=None, info=None):
    """Minimise f(P) with torch.optim.LBFGS (strong-Wolfe line search, lr = 1): torch does the two-loop recursion on the [C, E + 1]
    vectors, every pass over the features is ProbeObjective's.  init warm-starts (default: zeros); objective: a ProbeObjective to
    reuse (its l2 is set to `l2`); info: a dict that receives evals, iterations and the final loss.  -> P fp32 [C, E + 1]."""
    obj = objective if objective is not None else ProbeObjective(X, y, num_classes, l2, chunk_rows)
    obj.l2 = float(l2)
    with torch.cuda.device(obj.dev):
        P = torch.zeros(obj.C, obj.E + 1, dtype=F32, device=obj.dev) if init is None else init.detach().to(obj.dev, F32).clone()
        if tuple(P.shape) != (obj.C, obj.E + 1):
            raise ValueError(f"init must be [{obj.C}, {obj.E + 1}]")
        P.requires_grad_(True)
        opt = torch.optim.LBFGS([P], lr=1, max_iter=int(max_iter), history_size=int(history), tolerance_grad=tol_grad,
                                tolerance_change=tol_change, line_search_fn="strong_wolfe")
        before = obj.evals

        def closure():
            loss, grad = obj.value_and_grad(P.detach(), loss64=True)     # the line search compares the loss as it was folded: in double
            P.grad = grad
            return loss
        final = opt.step(closure)
        obj.check_labels()
        if info is not None:
            st = opt.state[P]
            info.update(evals=obj.evals - before, iterations=int(st.get("n_iter", 0)), first_loss=float(final))
        return P.detach()


def score_counts(pred, rank, y, num_classes, metric="accuracy"):
    """pred / rank (predict's) and labels -> dict(top1, top5, n), in percent.  "accuracy": hits / rows; "mean_per_class": the mean over
    the classes that occur of each class's own hit rate."""
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: one of {METRICS}")
    y = torch.as_tensor(y).cpu().long()
    hit1, hit5 = (pred.cpu().long() == y).double(), (rank.cpu() < 5).double()
    n = y.numel()
    if metric == "accuracy":
        return dict(top1=100.0 * hit1.sum().item() / max(n, 1), top5=100.0 * hit5.sum().item() / max(n, 1), n=n)
    cnt = torch.bincount(y, minlength=num_classes).double()
    seen = cnt > 0
    per = [(torch.bincount(y, weights=h, minlength=num_classes)[seen] / cnt[seen]).mean().item() for h in (hit1, hit5)]
    return dict(top1=100.0 * per[0], top5=100.0 * per[1], n=n)


def score(P, X, y, metric="accuracy", chunk_rows=65536):
    """Top-1 / top-5 of the classifier P on (X, y) -> dict(top1, top5, n), in percent."""
    pred, rank = predict(P, X, y, chunk_rows)
    return score_counts(pred, rank, y, P.shape[0], metric)


def sweep(Xtr, ytr, Xval, yval, num_classes, l2_grid, refit=False, metric="accuracy", fit_fn=None, score_fn=None, **fit_kw):
    """Fit at every l2 of the grid, strongest penalty first, each point warm-started from the previous one's P; choose by validation
    top-1, the smaller l2 on ties.  -> dict(best_l2, per_l2=[dict(l2, top1, top5, evals, P)] in grid order (descending), P).
    refit=True refits on train + val at the best point, warm-started from its P.  fit_fn / score_fn replace fit / score (tests)."""
    grid = sorted({float(v) for v in l2_grid}, reverse=True)
    if not grid:
        raise ValueError("sweep: an empty l2 grid")
    obj = ProbeObjective(Xtr, ytr, num_classes, grid[0], fit_kw.pop("chunk_rows", 65536)) if fit_fn is None else None
    fit_fn, score_fn = fit_fn or fit, score_fn or score
    per, best, P = [], None, None
    for l2 in grid:
        info = {}
        P = fit_fn(Xtr, ytr, num_classes, l2, init=P, objective=obj, info=info, **fit_kw)
        s = score_fn(P, Xval, yval, metric=metric)
        per.append(dict(l2=l2, top1=s["top1"], top5=s["top5"], evals=info.get("evals"), P=P))
        if best is None or s["top1"] >= best[0]:          # descending grid: >= keeps the smaller l2 on ties
            best = (s["top1"], l2, P)
    _, best_l2, bestP = best
    if refit:
        Xall = torch.cat([Xtr, Xval])
        yall = torch.cat([torch.as_tensor(ytr).to(Xall.device), torch.as_tensor(yval).to(Xall.device)])
        bestP = fit_fn(Xall, yall, num_classes, best_l2, init=bestP, objective=None, info={}, **fit_kw)
    return dict(best_l2=best_l2, per_l2=per, P=bestP)


# ---------------------------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------------------------
def weights_hash(model):
    """sha256 over the model's state_dict (names, shapes, bytes): the cache key's checkpoint part.  Remembered on the model for as
    long as no tensor of it is written or replaced (the stamp the engine's refresh() goes by: storage address and version counter)."""
    sd = model.state_dict()
    stamp = tuple((k, v.data_ptr(), v._version) for k, v in sd.items())
    memo = getattr(model, "_probe_weights_hash", None)
    if memo is not None and memo[0] == stamp:
        return memo[1]
    digest = _hash_state_dict(sd)
    try:
        model._probe_weights_hash = (stamp, digest)
    except AttributeError:
        pass
    return digest


def _hash_state_dict(sd):
    h = hashlib.sha256()
    for k, v in sorted(sd.items()):
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        t = v.detach().cpu().contiguous().reshape(-1)           # (reshape: a 0-dim tensor has no byte view)
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def cache_key(model, items, features, normalize, size):
    h = hashlib.sha256(weights_hash(model).encode())
    h.update(repr((features, bool(normalize), int(size), [(os.path.basename(p), c) for p, c in items])).encode())
    return h.hexdigest()


def save_cache(path, key, X, y, classnames):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp.npz"
    np.savez(tmp, key=np.array(key), X=X.detach().cpu().numpy(), y=torch.as_tensor(y).cpu().numpy().astype(np.int64),
             classnames=np.array(list(classnames)))
    os.replace(tmp, path)


def load_cache(path, key):
    """-> (X fp32 numpy, y int64 numpy, classnames) or None when the file is missing or was written under another key."""
    if not os.path.exists(path):
        return None
    with np.load(path, allow_pickle=False) as z:
        if str(z["key"]) != key:
            return None
        return z["X"].astype(np.float32), z["y"].astype(np.int64), [str(c) for c in z["classnames"]]


@torch.no_grad()
def extract_features(model, root, batch_size=64, features="proj", normalize=False, workers=None, processes=None, max_images=None,
                     cache=None, size=224, mean=zeroshot.IMAGENET_MEAN, std=zeroshot.IMAGENET_STD, device="cuda", stats=None):
    """Image features of an ImageFolder tree -> (X fp32 [N, E] on the device, y int64 [N] on the host, classnames): rows in
    zeroshot.image_folder's order, decoded by zeroshot.ImagePipeline (no augmentation), features="proj" = the projected image
    embedding encode_image(norm=normalize).  max_images: a strided subset.  cache: path of an .npz that is written after the run and
    read instead of it next time, keyed by the weights' hash, the file list and the options.  stats: a dict that receives
    images, seconds, images_per_s and from_cache."""
    if features not in FEATURES:
        raise ValueError(f"features {features!r}: one of {FEATURES}")
    hip.require_gpu()
    classes, items = zeroshot.image_folder(root)
    if max_images:
        items = items[::max(1, len(items) // max_images)][:max_images]
    if not items:
        raise ValueError(f"no images under {root}")
    dev = torch.device(device)
    t0 = time.perf_counter()
    key = cache_key(model, items, features, normalize, size) if cache else None
    hit = load_cache(cache, key) if cache else None
    if hit is not None:
        X, y = torch.from_numpy(hit[0]).to(dev), torch.from_numpy(hit[1])
    else:
        if processes is None:
            cores = zeroshot.effective_cores()
            processes = min(32, cores // 2) if (workers is None and len(items) >= 2048 and cores >= 8) else 0
        pipe = zeroshot.ImagePipeline(items, batch_size, dev, size, mean, std, workers, processes=processes)
        rows = []
        try:
            for x, _, _ in pipe:
                rows.append(model.encode_image(x, norm=normalize).float())
        finally:
            pipe.close()
        X, y = torch.cat(rows), torch.tensor([c for _, c in items], dtype=torch.int64)
        torch.cuda.synchronize(dev)
        if cache:
            save_cache(cache, key, X, y, classes)
    if stats is not None:
        el = time.perf_counter() - t0
        stats.update(images=len(items), seconds=el, images_per_s=len(items) / max(el, 1e-9), from_cache=hit is not None)
    return X, y, classes


def evaluate(model, train_root, val_root, l2=None, csk=0.316, l2_grid=None, metric="accuracy", batch_size=64, features="proj",
             normalize=False, workers=None, processes=None, max_images=None, cache=None, max_iter=1000, chunk_rows=65536,
             size=224, mean=zeroshot.IMAGENET_MEAN, std=zeroshot.IMAGENET_STD, log=print):
    """The whole protocol: features of both trees, one fit (l2, or Csk -> l2 = 1 / (Csk N)) or a sweep over l2_grid (every fifth
    training row held out for the choice, then a refit on all of them), scores on both.  cache: a directory for the two feature
    files.  -> dict(train_top1, train_top5, val_top1, val_top5, l2, csk, evals, images_per_s, fit_s, n_train, n_val, classes, P)."""
    kw = dict(batch_size=batch_size, features=features, normalize=normalize, workers=workers, processes=processes,
              max_images=max_images, size=size, mean=mean, std=std)
    st_tr, st_va = {}, {}
    Xtr, ytr, classes = extract_features(model, train_root, cache=os.path.join(cache, "train.npz") if cache else None, stats=st_tr, **kw)
    Xva, yva, classes_va = extract_features(model, val_root, cache=os.path.join(cache, "val.npz") if cache else None, stats=st_va, **kw)
    if classes != classes_va:
        raise ValueError(f"class directories differ: {len(classes)} under {train_root}, {len(classes_va)} under {val_root}")
    C, N = len(classes), Xtr.shape[0]
    log(f"=> features: {N} train + {Xva.shape[0]} val rows of {Xtr.shape[1]}, {C} classes")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info, per = {}, None
    if l2_grid:
        hold = torch.arange(N) % 5 == 4
        sw = sweep(Xtr[~hold.to(Xtr.device)], ytr[~hold], Xtr[hold.to(Xtr.device)], ytr[hold], C, l2_grid, metric=metric,
                   max_iter=max_iter, chunk_rows=chunk_rows)
        l2, per = sw["best_l2"], sw["per_l2"]
        init = torch.zeros(C, Xtr.shape[1] + 1, dtype=F32, device=Xtr.device)
        init.copy_(sw["P"])
        evals_sweep = sum(p["evals"] or 0 for p in per)
        P = fit(Xtr, ytr, C, l2, max_iter=max_iter, init=init, chunk_rows=chunk_rows, info=info)
        info["evals"] += evals_sweep
    else:
        l2 = float(l2) if l2 is not None else l2_from_csk(csk, N)
        P = fit(Xtr, ytr, C, l2, max_iter=max_iter, chunk_rows=chunk_rows, info=info)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    tr, va = score(P, Xtr, ytr, metric, chunk_rows), score(P, Xva, yva, metric, chunk_rows)
    imgs, secs = st_tr["images"] + st_va["images"], st_tr["seconds"] + st_va["seconds"]
    log("=> linear probe ({}): train@1 {:.3f}%  val@1 {:.3f}%  val@5 {:.3f}%  l2 {:.3e} (Csk {:.4g})  {} evaluations, fit {:.2f} s, "
        "{:.1f} images/s".format(metric, tr["top1"], va["top1"], va["top5"], l2, csk_from_l2(l2, N), info["evals"], fit_s,
                                 imgs / max(secs, 1e-9)))
    return dict(train_top1=tr["top1"], train_top5=tr["top5"], val_top1=va["top1"], val_top5=va["top5"], l2=l2, csk=csk_from_l2(l2, N),
                evals=info["evals"], images_per_s=imgs / max(secs, 1e-9), fit_s=fit_s, n_train=N, n_val=int(Xva.shape[0]),
                classes=C, metric=metric, per_l2=per, P=P)
