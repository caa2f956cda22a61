"""Linear probing on a real MI355X (msclip_amd/linear_probe.py, include/msclip_ext5.h): one evaluation of the objective against
fp64, chunking, repeatability, the L-BFGS fit against the scikit-learn fixture, held-out prediction, the sweep, and the whole
protocol on a generated image folder.

Bounds.  tests/probe_ref.py emulates the device recipe (bf16 hi/lo splits of X, W and G, three-term products) with exact
accumulation; its distance from fp64 on the SAME inputs is the cost of the recipe itself.  The device adds fp32 accumulation over
K = 3 E and over the rows, estimated at the same order, so it must stay within K_EMU = 8 times the emulation's error -- for
|loss - loss64| / loss64 and for max|g - g64| / max|g64|, the latter with a floor of 1e-6 max|g64| (fp32 roundings of the stored
gradient).  The measured ratios are in profiles/linear_probe_accuracy.md.  The fit: the emulated recipe driven by the same L-BFGS on
the CPU stops 0.8e-3 .. 1.2e-3 from the fp64 optimum; 5e-3 leaves five times that for the spread of the stopping point."""
import functools
import os

import numpy as np
import pytest
import torch

import probe_ref as R
from conftest import synth_sd
from msclip_amd import hip, linear_probe as LP, zeroshot

pytestmark = pytest.mark.gpu
K_EMU = 8.0
GRAD_FLOOR = 1e-6
FIT_TOL = 5e-3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_probe_fixture.npz")
B32 = "b32-yfcc-msclips"
L2_EVAL = 1e-3
#        R     E    C     chunk  target max|S| (None: features as drawn)
CASES = {"chunks_ragged_tail": (1000, 512, 130, 256, None),
         "mostly_padding": (77, 64, 5, 16384, None),
         "wide": (256, 512, 1000, 16384, None),
         "large_logits": (1000, 512, 130, 256, 80.0)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the fp64 values and the emulation's error, computed once and shared."""
    N, E, C, chunk, smax = CASES[name]
    g = torch.Generator().manual_seed(17)
    X = torch.randn(N, E, generator=g)
    y = torch.randint(0, C, (N,), generator=g)
    y[0], y[1] = 0, C - 1
    P = (0.05 * torch.randn(C, E + 1, generator=g)).float()
    assert float(P[:, E].abs().min()) > 0                                    # a non-zero bias
    if smax is not None:
        S = X.double() @ P[:, :E].double().t() + P[:, E].double()
        X = X * (smax / float(S.abs().max()))
    X = X.float()
    loss64, g64 = R.objective(P, X, y, L2_EVAL)
    eloss, eg = R.emulate(P, X, y, L2_EVAL)
    S64 = X.double() @ P[:, :E].double().t() + P[:, E].double()
    return dict(X=X, y=y, P=P, C=C, E=E, chunk=chunk, loss64=float(loss64), g64=g64, S64=S64,
                emu_loss=abs(float(eloss - loss64)) / float(loss64), emu_grad=float((eg - g64).abs().max() / g64.abs().max()))


def _evaluate(c, chunk=None):
    obj = LP.ProbeObjective(c["X"].cuda(), c["y"], c["C"], L2_EVAL, chunk_rows=chunk or c["chunk"])
    loss, grad = obj.value_and_grad(c["P"].cuda())
    return obj, loss, grad


def _errors(c, loss, grad):
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32 and loss.dim() == 0 and grad.shape == c["g64"].shape
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    le = abs(float(loss.double().cpu()) - c["loss64"]) / c["loss64"]
    ge = float((grad.double().cpu() - c["g64"]).abs().max() / c["g64"].abs().max())
    return le, ge


def _within(c, le, ge, what):
    print(f"{what}: loss error {le:.3e} (emulation {c['emu_loss']:.3e}, ratio {le / c['emu_loss']:.2f}); gradient error {ge:.3e} of "
          f"max|g| (emulation {c['emu_grad']:.3e}, ratio {ge / c['emu_grad']:.2f})")
    assert le <= K_EMU * c["emu_loss"], (le, c["emu_loss"])
    assert ge <= max(K_EMU * c["emu_grad"], GRAD_FLOOR), (ge, c["emu_grad"])


# ---------------------------------------------------------------------------- 1. one evaluation against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_one_evaluation_against_fp64(gpu_device, name):
    c = _case(name)
    C, N = c["C"], c["X"].shape[0]
    assert int(c["y"].min()) == 0 and int(c["y"].max()) == C - 1
    if CASES[name][4] is not None:
        assert 79.0 <= float(c["S64"].abs().max()) <= 81.0
    obj, loss, grad = _evaluate(c)
    _within(c, *_errors(c, loss, grad), what=name)
    # padded classes: G's columns [C, Cpad) are exactly zero (the buffers hold the last chunk), every prediction is a class
    last = N - (N - 1) // obj.chunk * obj.chunk
    assert obj.Cpad % 16 == 0 and obj.Cpad >= C
    if obj.Cpad > C:
        assert not bool(obj.Gh[:last, C:].float().abs().sum()) and not bool(obj.Gl[:last, C:].float().abs().sum())
    assert bool(torch.isfinite(obj.Gh[:last].float()).all()) and bool(torch.isfinite(obj.Gl[:last].float()).all())
    pred, rank = obj.predict(c["P"].cuda(), c["X"].cuda(), c["y"])
    pred, rank = pred.cpu().long(), rank.cpu().long()
    assert int(pred.min()) >= 0 and int(pred.max()) < C and int(rank.min()) >= 0 and int(rank.max()) < C
    S = c["S64"]
    top = S.sort(1, descending=True).values
    clear = (top[:, 0] - top[:, 1]) >= 1e-3 * float(S.abs().max())
    assert torch.equal(pred[clear], S.argmax(1)[clear]) and float(clear.double().mean()) > 0.9
    obj.check_labels()


def test_labels_out_of_range(gpu_device):
    c = _case("mostly_padding")
    bad = c["y"].clone()
    bad[3], bad[40] = c["C"] + 3, -1
    with pytest.raises(ValueError):                                          # host labels: refused before anything runs
        LP.ProbeObjective(c["X"].cuda(), bad, c["C"], L2_EVAL)
    obj = LP.ProbeObjective(c["X"].cuda(), bad.cuda(), c["C"], L2_EVAL)      # device labels: clamped and counted by the kernel
    loss, grad = obj.value_and_grad(c["P"].cuda())
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and int(obj.bad_part.sum()) == 2
    with pytest.raises(ValueError):
        obj.check_labels()


def test_split_bf16_is_hi_and_lo(gpu_device):
    g = torch.Generator().manual_seed(2)
    for M, Cc in ((37, 64), (5, 7), (300, 512)):                             # 16-byte path, element path (odd width), more than one block
        x = (torch.randn(M, Cc, generator=g) * 3).cuda()
        out = hip.split_bf16(x)
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
        assert torch.equal(out[:, :Cc].view(torch.int16), hi.view(torch.int16))
        assert torch.equal(out[:, Cc:].view(torch.int16), lo.view(torch.int16))


# ---------------------------------------------------------------------------- 2. chunking
@pytest.mark.parametrize("chunk", [256, 512, 16384])
def test_chunking(gpu_device, chunk):
    """Every chunk size stays within test 1's bound.  The results are NOT bitwise equal across chunk sizes in general: the chunk
    partials of dW and db are added in chunk order, another grouping of the rows; the loss, folded in double from the same 32-row
    partials, happens to be."""
    c = _case("chunks_ragged_tail")
    _, loss, grad = _evaluate(c, chunk)
    _within(c, *_errors(c, loss, grad), what=f"chunk_rows {chunk}")


# ---------------------------------------------------------------------------- 3. repeatability
def test_two_evaluations_are_bitwise_equal(gpu_device):
    c = _case("chunks_ragged_tail")
    obj, loss, grad = _evaluate(c)
    pred, rank = obj.predict(c["P"].cuda(), c["X"].cuda(), c["y"])
    loss2, grad2 = obj.value_and_grad(c["P"].cuda())
    pred2, rank2 = obj.predict(c["P"].cuda(), c["X"].cuda(), c["y"])
    _, loss3, grad3 = _evaluate(c)                                            # a fresh objective: other buffers
    for a, b in ((loss, loss2), (grad, grad2), (loss, loss3), (grad, grad3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(pred, pred2) and torch.equal(rank, rank2)


# ---------------------------------------------------------------------------- 4. the fit against the fixture
@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _fitted(k):
    fx = _fixture()
    info = {}
    P = LP.fit(torch.from_numpy(fx["X"]).cuda(), torch.from_numpy(fx["y"]), 7, float(fx["l2"][k]), max_iter=1000, info=info)
    return P.cpu(), info


@pytest.mark.parametrize("k", [0, 1])
def test_fit_against_the_fixture(gpu_device, k):
    fx = _fixture()
    P, info = _fitted(k)
    l2, Psk = float(fx["l2"][k]), torch.from_numpy(fx["P"][k])
    X, y = torch.from_numpy(fx["X"]), torch.from_numpy(fx["y"])
    d = R.rel_distance(P, Psk)
    f, fsk = float(R.objective(P, X, y, l2)[0]), float(R.objective(Psk, X, y, l2)[0])
    print(f"l2 {l2}: ||P - P_sk|| / ||P_sk|| = {d:.3e} after {info['evals']} evaluations; fp64 objective {f:.12f} vs {fsk:.12f} "
          f"({(f - fsk) / fsk:.2e} relative)")
    assert P.dtype == torch.float32 and tuple(P.shape) == (7, 65)
    assert d <= FIT_TOL
    assert abs(f - fsk) <= 1e-6 * fsk


# ---------------------------------------------------------------------------- 5. held-out prediction
@pytest.mark.parametrize("k", [0, 1])
def test_held_out_prediction(gpu_device, k):
    fx = _fixture()
    S, yval = torch.from_numpy(fx["val_logits"][k]), torch.from_numpy(fx["yval"])
    P, Xval = torch.from_numpy(fx["P"][k]).float().cuda(), torch.from_numpy(fx["Xval"]).cuda()
    pred, rank = LP.predict(P, Xval, yval)
    pred, rank = pred.cpu().long(), rank.cpu().long()
    thr = 1e-3 * float(S.abs().max())
    top = S.sort(1, descending=True).values
    clear = (top[:, 0] - top[:, 1]) >= thr
    assert float((~clear).double().mean()) <= 0.01
    assert torch.equal(pred[clear], S.argmax(1)[clear])
    # the rank: rows whose label's logit is at least the margin away from every other logit
    gap = (S - S[torch.arange(300), yval][:, None]).abs()
    gap[torch.arange(300), yval] = float("inf")
    clear_r = gap.min(1).values >= thr
    rank64 = (S > S[torch.arange(300), yval][:, None]).sum(1)
    assert float((~clear_r).double().mean()) <= 0.01
    assert torch.equal(rank[clear_r], rank64[clear_r]) and torch.equal(rank[clear_r] < 5, rank64[clear_r] < 5)
    # score = the same numbers recomputed from pred / rank on the host
    hit1, hit5 = (pred == yval).numpy(), (rank < 5).numpy()
    acc = LP.score(P, Xval, yval)
    assert acc == dict(top1=pytest.approx(100.0 * hit1.mean(), abs=1e-9), top5=pytest.approx(100.0 * hit5.mean(), abs=1e-9), n=300)
    mpc = LP.score(P, Xval, yval, metric="mean_per_class")
    yv = yval.numpy()
    assert mpc["top1"] == pytest.approx(100.0 * np.mean([hit1[yv == c].mean() for c in range(7)]), abs=1e-9)
    assert mpc["top5"] == pytest.approx(100.0 * np.mean([hit5[yv == c].mean() for c in range(7)]), abs=1e-9)
    assert 60.0 <= acc["top1"] <= 90.0


# ---------------------------------------------------------------------------- 6. the sweep
def test_sweep_on_the_fixture(gpu_device):
    fx = _fixture()
    X, y = torch.from_numpy(fx["X"]).cuda(), torch.from_numpy(fx["y"])
    Xval, yval = torch.from_numpy(fx["Xval"]).cuda(), torch.from_numpy(fx["yval"])
    grid = [1e-3, 1e-1, 1e-2]
    out = LP.sweep(X, y, Xval, yval, 7, grid, max_iter=1000)
    assert [p["l2"] for p in out["per_l2"]] == [1e-1, 1e-2, 1e-3]
    for p in out["per_l2"]:
        cold = _fitted({1e-3: 0, 1e-2: 1}[p["l2"]])[0] if p["l2"] < 1e-1 else LP.fit(X, y, 7, p["l2"], max_iter=1000).cpu()
        d = R.rel_distance(p["P"].cpu(), cold)
        print(f"l2 {p['l2']}: warm-started vs cold fit {d:.3e}, val top-1 {p['top1']:.2f}, {p['evals']} evaluations")
        assert d <= FIT_TOL
        assert p["top1"] == pytest.approx(LP.score(p["P"], Xval, yval)["top1"])
    best = max(out["per_l2"], key=lambda p: (p["top1"], -p["l2"]))           # the best top-1, the smaller l2 on ties
    assert out["best_l2"] == best["l2"] and torch.equal(out["P"], best["P"])


# ---------------------------------------------------------------------------- 7. end to end
def _image_tree(root, per_class, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    colours = {"amber": (220, 160, 30), "blue": (30, 60, 200), "green": (40, 180, 70)}
    for name, rgb in colours.items():
        os.makedirs(os.path.join(root, name))
        for i in range(per_class):
            px = np.clip(np.asarray(rgb)[None, None, :] + rng.normal(0, 25, (32, 32, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(px).save(os.path.join(root, name, f"{i:02d}.png"))


def test_end_to_end_on_a_generated_folder(gpu_device, tmp_path):
    from PIL import Image
    from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
    from msclip_amd.config import named_config
    train_root, val_root = str(tmp_path / "train"), str(tmp_path / "val")
    _image_tree(train_root, 8, 1)
    _image_tree(val_root, 4, 2)
    model = get_clip_model(named_config(B32))
    model.load_state_dict(synth_sd(B32), strict=True)
    model = model.cuda().eval()
    stats = {}
    cache = str(tmp_path / "cache" / "train.npz")
    X, y, classes = LP.extract_features(model, train_root, batch_size=8, cache=cache, stats=stats)
    assert classes == ["amber", "blue", "green"] and tuple(X.shape) == (24, 512) and X.dtype == torch.float32 and X.is_cuda
    assert y.tolist() == [0] * 8 + [1] * 8 + [2] * 8 and y.dtype == torch.int64 and not stats["from_cache"]
    _, items = zeroshot.image_folder(train_root)
    for b in range(3):                                                        # the same batches through encode_image
        batch = torch.stack([zeroshot.preprocess(Image.open(p)) for p, _ in items[8 * b:8 * b + 8]]).cuda()
        ref = model.encode_image(batch, norm=False).float()
        assert torch.equal(X[8 * b:8 * b + 8].view(torch.int32), ref.view(torch.int32))
    X2, y2, _ = LP.extract_features(model, train_root, batch_size=8, cache=cache, stats=stats)
    assert stats["from_cache"] and torch.equal(X2.view(torch.int32), X.view(torch.int32)) and torch.equal(y2, y)
    res = LP.evaluate(model, train_root, val_root, l2=1e-2, batch_size=8, max_iter=100, cache=str(tmp_path / "cache"), log=lambda s: None)
    Xv, yv, _ = LP.extract_features(model, val_root, batch_size=8)
    P = LP.fit(X, y, 3, 1e-2, max_iter=100)
    tr, va = LP.score(P, X, y), LP.score(P, Xv, yv)
    assert (res["train_top1"], res["train_top5"], res["val_top1"], res["val_top5"]) == (tr["top1"], tr["top5"], va["top1"], va["top5"])
    assert res["n_train"] == 24 and res["n_val"] == 12 and res["classes"] == 3 and res["l2"] == 1e-2 and res["evals"] >= 1
    assert res["fit_s"] > 0 and res["images_per_s"] > 0 and torch.equal(res["P"], P)
