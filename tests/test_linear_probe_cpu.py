"""Linear probing (msclip_amd/linear_probe.py, include/msclip_ext5.h) without a GPU: the fifth extension header's binding, the
library's exports and argument validation (which runs on the host, before any launch), the fp64 reference and the emulation of the
device recipe (tests/probe_ref.py), the scikit-learn fixture, and the host logic (sweep's selection, the l2 <-> Csk mapping, the
feature cache, folder order -> labels)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import probe_ref as R
from msclip_amd import abi, hip, linear_probe as LP, zeroshot

VP, CI, CF, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_probe_fixture.npz")


def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------- the extension header
def test_probe_header_binding():
    main = abi.load()
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    ext4 = abi.load(abi.EXT4_HEADER, abi.EXT4_VERSION_MACRO, known=tuple(main.structs) + tuple(ext3.structs))
    ext5 = abi.load(abi.EXT5_HEADER, abi.EXT5_VERSION_MACRO)
    assert os.path.basename(abi.EXT5_HEADER) == "msclip_ext5.h" and ext5.version == 1 == hip.EXT5_ABI_VERSION
    assert not ext5.structs
    assert ext5.protos == {
        "msclip_probe_ce_rows": (CI, [VP, CI, VP, VP, CI, CI, CI, CF, VP, VP, VP, CI, VP, VP, CI, VP, VP, VP, VP]),
        "msclip_probe_loss_fold": (CI, [VP, LL, LL, VP, VP]),
        "msclip_split_bf16": (CI, [VP, CI, VP, CI, LL, CI, VP]),
        "msclip_ext5_abi_version": (CI, []),
    }
    assert hip.EXT5_EXPORTS == tuple(ext5.protos)
    others = set(main.protos) | set(ext.protos) | set(ext2.protos) | set(ext3.protos) | set(ext4.protos)
    assert not set(ext5.protos) & others
    assert (set(hip.EXPORTS) | set(hip.EXT_EXPORTS) | set(hip.EXT2_EXPORTS) | set(hip.EXT3_EXPORTS) | set(hip.EXT4_EXPORTS)) == others
    assert [row[0] for row in hip._BOUND] == ["_ABI", "_EXT", "_EXT2", "_EXT3", "_EXT4", "_EXT5"]
    # the older headers are what they were (tests/test_nonfinite_cpu.py)
    assert main.version == 9 and len(main.protos) == 107 and ext.version == 1 and ext2.version == 1 and ext3.version == 1
    assert len(ext.protos) == 2 and len(ext2.protos) == 4 and len(ext3.protos) == 4
    assert ext4.version == 1 and len(ext4.protos) == 4
    assert ctypes.sizeof(hip.AdamwTensor) == 64 and ctypes.sizeof(hip.LambTensor) == 72
    assert hip.PROBE_ROWS == 32
    with open(abi.EXT5_HEADER) as f:
        assert "#define MSCLIP_PROBE_ROWS 32" in f.read()


def test_library_exports_and_rejections():
    """Every MSCLIP_EINVAL rule on fake non-null pointers: a call that got past its checks would launch on them."""
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.EXT5_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_ext5_abi_version() == 1
    p, odd, four = VP(0x10000), VP(0x10002), VP(0x10004)

    def rows(S=p, lds=16, bias=p, labels=p, Rn=8, C=5, Cpad=16, lse=p, gh=p, gl=p, ldg=16, lp=p, cp=p, ldp=16, pred=p, rank=p,
             bad=p):
        return L.msclip_probe_ce_rows(S, lds, bias, labels, Rn, C, Cpad, 0.125, lse, gh, gl, ldg, lp, cp, ldp, pred, rank, bad, None)
    assert rows(S=None) == -1                                                 # null
    for name in ("S", "bias", "labels", "lse", "gh", "gl", "lp", "cp", "pred", "rank", "bad"):
        assert rows(**{name: odd}) == -1, name                               # misaligned
    assert rows(lp=four) == -1                                               # the loss partials are doubles: 8 bytes
    assert rows(C=1) == -1 and rows(C=0) == -1                               # C < 2
    assert rows(C=17) == -1 and rows(Cpad=4) == -1                           # Cpad < C
    assert rows(Rn=0) == -1 and rows(Rn=-5) == -1                            # R <= 0
    assert rows(lds=15) == -1                                                # lds < Cpad
    assert rows(ldg=15) == -1 and rows(ldp=15) == -1                         # ldg, ldp < Cpad
    assert rows(gl=None) == -1 and rows(cp=None) == -1                       # G needs both halves and the column-sum partials
    assert rows(gh=None) == -1 and rows(gh=None, gl=None) == -1              # ... and without G neither of them
    assert rows(labels=None) == -1                                           # G, loss, rank, the count need labels
    assert rows(labels=None, gh=None, gl=None, cp=None, lp=None, rank=p, bad=None) == -1
    assert rows(labels=None, gh=None, gl=None, cp=None, lp=p, rank=None, bad=None) == -1
    # the loss fold
    for args in ((None, 4, 4, p), (p, 4, 4, None), (p, 0, 4, p), (p, -1, 4, p), (p, 4, 0, p), (four, 4, 4, p), (p, 4, 4, four),
                 (odd, 4, 4, p)):
        assert L.msclip_probe_loss_fold(*args, None) == -1, args
    # the split
    for args in ((None, 8, p, 16, 4, 8), (p, 8, None, 16, 4, 8), (odd, 8, p, 16, 4, 8), (p, 8, odd, 16, 4, 8), (p, 8, p, 16, 0, 8),
                 (p, 8, p, 16, 4, 0), (p, 7, p, 16, 4, 8), (p, 8, p, 15, 4, 8)):
        assert L.msclip_split_bf16(*args, None) == -1, args


# ---------------------------------------------------------------------------- the reference and the emulation
def _problem(N, E, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(N, E, generator=g) * scale).float()
    y = torch.randint(0, C, (N,), generator=g)
    y[0], y[1] = 0, C - 1
    P = (0.05 * torch.randn(C, E + 1, generator=g)).float()
    return X, y, P


def test_reference_gradient_is_autograd():
    for N, E, C, l2 in ((50, 16, 5, 1e-2), (77, 64, 7, 0.0), (40, 8, 2, 1.0)):
        X, y, P = _problem(N, E, C, 3)
        loss, grad = R.objective(P, X, y, l2)
        aloss, agrad = R.objective_autograd(P, X, y, l2)
        assert abs(float(loss - aloss)) <= 1e-13 * abs(float(aloss))
        assert (grad - agrad).abs().max().item() <= 1e-14 * max(1.0, agrad.abs().max().item())


def test_emulation_error_is_printed_and_sane():
    """The recipe's own error: three-term bf16 products leave ~2^-17 per operand pair (the dropped lo.lo term and the rounding of
    lo), so the gradient sits ~1e-6 .. 1e-5 of max|g| from fp64 and the loss, a mean over the rows, far closer."""
    for N, E, C in ((1000, 512, 130), (77, 64, 5), (256, 512, 1000)):
        X, y, P = _problem(N, E, C, 11)
        loss, grad = R.objective(P, X, y, 1e-3)
        eloss, egrad = R.emulate(P, X, y, 1e-3)
        le = abs(float(eloss - loss)) / float(loss)
        ge = (egrad - grad).abs().max().item() / grad.abs().max().item()
        print(f"emulation vs fp64 at N={N} E={E} C={C}: loss {le:.2e} relative, gradient {ge:.2e} of max|g|")
        assert le < 1e-6 and 1e-8 < ge < 5e-5


def test_centring():
    P = torch.randn(4, 6, dtype=torch.float64)
    Q = P.clone()
    Q[:, -1] += 3.5
    assert R.rel_distance(P, Q) < 1e-15 and abs(float(R.centre(P)[:, -1].mean())) < 1e-15
    X, y, _ = _problem(30, 5, 4, 1)
    assert abs(float(R.objective(P, X, y, 0.1)[0] - R.objective(Q, X, y, 0.1)[0])) < 1e-12


# ---------------------------------------------------------------------------- the fixture
def test_fixture_shape_and_margin_cap():
    fx = _fixture()
    assert fx["X"].shape == (600, 64) and fx["X"].dtype == np.float32 and fx["Xval"].shape == (300, 64)
    assert fx["P"].shape == (2, 7, 65) and fx["val_logits"].shape == (2, 300, 7) and list(fx["l2"]) == [1e-3, 1e-2]
    assert os.path.getsize(FIXTURE) < 400 << 10
    for k in range(2):
        S = fx["val_logits"][k]
        P = torch.from_numpy(fx["P"][k])
        again = torch.from_numpy(fx["Xval"]).double() @ P[:, :64].t() + P[:, 64]
        assert np.allclose(again.numpy(), S, rtol=0, atol=1e-12)
        acc = float(np.mean(S.argmax(1) == fx["yval"]))
        assert 0.6 <= acc <= 0.9, acc                                     # a fixture that is always right tests no prediction
        top = np.sort(S, 1)
        low = top[:, -1] - top[:, -2] < 1e-3 * np.abs(S).max()
        assert low.mean() <= 0.01                                          # the rows the GPU test may leave out


def test_fixture_is_the_minimum_by_lbfgs_in_fp64():
    fx = _fixture()
    X, y = torch.from_numpy(fx["X"]), torch.from_numpy(fx["y"])
    for k, l2 in enumerate(fx["l2"]):
        Psk = torch.from_numpy(fx["P"][k])
        P = R.fit_lbfgs(X, y, 7, float(l2))
        d = R.rel_distance(P, Psk)
        f, fsk = float(R.objective(P, X, y, float(l2))[0]), float(R.objective(Psk, X, y, float(l2))[0])
        print(f"l2 {l2}: fp64 L-BFGS vs scikit-learn {d:.2e}, objective {f:.12f} vs {fsk:.12f}")
        assert d <= 1e-3 and abs(f - fsk) <= 1e-8 * fsk


def test_fixture_is_what_sklearn_gives():
    pytest.importorskip("sklearn")
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_golden_probe", os.path.join(os.path.dirname(os.path.dirname(FIXTURE)), "..", "tools", "make_golden_probe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    fx = _fixture()
    X, y, Xval, yval = tool.make_data(int(fx["seed"]), float(fx["sep"]))
    assert np.array_equal(X, fx["X"]) and np.array_equal(y, fx["y"]) and np.array_equal(Xval, fx["Xval"]) and np.array_equal(yval, fx["yval"])
    for k, l2 in enumerate(fx["l2"]):
        assert tool.solve(X, y, float(l2)).shape == (7, 65)
        assert R.rel_distance(torch.from_numpy(tool.solve(X, y, float(l2))), torch.from_numpy(fx["P"][k])) <= 1e-3


# ---------------------------------------------------------------------------- host logic
def test_l2_csk_mapping():
    assert LP.l2_from_csk(0.316, 1000) == pytest.approx(1.0 / 316.0)
    assert LP.csk_from_l2(LP.l2_from_csk(0.316, 1281167), 1281167) == pytest.approx(0.316)
    assert LP.l2_from_csk(2.0, 50) == 0.01 and LP.csk_from_l2(0.01, 50) == 2.0


def test_sweep_selection_tie_rule_and_warm_start_order():
    calls = []
    top1 = {1.0: 50.0, 0.1: 70.0, 0.01: 70.0, 0.001: 60.0}

    def fit_fn(X, y, C, l2, init=None, objective=None, info=None, **kw):
        calls.append((l2, None if init is None else float(init[0]), X, kw))
        info["evals"] = 3
        return torch.tensor([l2], dtype=torch.float64)

    def score_fn(P, X, y, metric="accuracy"):
        assert X == "Xval" and y == "yval" and metric == "mean_per_class"
        return dict(top1=top1[float(P[0])], top5=99.0, n=4)
    out = LP.sweep("Xtr", "ytr", "Xval", "yval", 3, [0.01, 1.0, 0.001, 0.1, 0.1], metric="mean_per_class", fit_fn=fit_fn,
                   score_fn=score_fn, max_iter=7)
    assert [c[0] for c in calls] == [1.0, 0.1, 0.01, 0.001]                  # descending, duplicates once
    assert [c[1] for c in calls] == [None, 1.0, 0.1, 0.01]                   # each warm-started from the previous point
    assert all(c[2] == "Xtr" and c[3] == {"max_iter": 7} for c in calls)
    assert out["best_l2"] == 0.01 and float(out["P"][0]) == 0.01             # 70 twice: the smaller l2
    assert [p["l2"] for p in out["per_l2"]] == [1.0, 0.1, 0.01, 0.001] and [p["top1"] for p in out["per_l2"]] == [50.0, 70.0, 70.0, 60.0]
    assert all(p["evals"] == 3 and p["top5"] == 99.0 for p in out["per_l2"])
    with pytest.raises(ValueError):
        LP.sweep("Xtr", "ytr", "Xval", "yval", 3, [], fit_fn=fit_fn, score_fn=score_fn)


def test_score_counts_metrics():
    y = torch.tensor([0, 0, 0, 0, 1, 2])
    pred = torch.tensor([0, 0, 0, 1, 1, 0], dtype=torch.int32)
    rank = torch.tensor([0, 0, 0, 1, 0, 7], dtype=torch.int32)
    a = LP.score_counts(pred, rank, y, 4, "accuracy")
    assert a == dict(top1=pytest.approx(100 * 4 / 6), top5=pytest.approx(100 * 5 / 6), n=6)
    m = LP.score_counts(pred, rank, y, 4, "mean_per_class")                  # class 3 does not occur: not in the mean
    assert m == dict(top1=pytest.approx(100 * (0.75 + 1 + 0) / 3), top5=pytest.approx(100 * (1 + 1 + 0) / 3), n=6)
    with pytest.raises(ValueError):
        LP.score_counts(pred, rank, y, 4, "f1")


def test_cache_round_trip(tmp_path):
    model = torch.nn.Linear(3, 2)
    items = [("/a/x.png", 0), ("/a/y.png", 1)]
    key = LP.cache_key(model, items, "proj", False, 224)
    assert key == LP.cache_key(model, items, "proj", False, 224)
    assert key != LP.cache_key(model, items, "proj", True, 224) and key != LP.cache_key(model, items[:1], "proj", False, 224)
    X, y = torch.randn(2, 5), torch.tensor([0, 1])
    path = str(tmp_path / "sub" / "train.npz")
    assert LP.load_cache(path, key) is None
    LP.save_cache(path, key, X, y, ["cat", "dog"])
    Xc, yc, names = LP.load_cache(path, key)
    assert np.array_equal(Xc, X.numpy()) and Xc.dtype == np.float32 and np.array_equal(yc, y.numpy()) and names == ["cat", "dog"]
    with torch.no_grad():
        model.weight[0, 0] += 1.0                                            # other weights: another key, the file is not used
    assert LP.load_cache(path, LP.cache_key(model, items, "proj", False, 224)) is None


def test_image_folder_order_gives_the_labels(tmp_path):
    for d, files in (("zebra", ["b.png", "a.png"]), ("ant", ["2.jpg", "10.jpg", "note.txt"]), ("mole", ["m.PNG"])):
        os.makedirs(tmp_path / d)
        for f in files:
            (tmp_path / d / f).write_bytes(b"")
    (tmp_path / "stray.png").write_bytes(b"")
    classes, items = zeroshot.image_folder(str(tmp_path))
    assert classes == ["ant", "mole", "zebra"]
    assert [(os.path.relpath(p, tmp_path), c) for p, c in items] == [
        ("ant/10.jpg", 0), ("ant/2.jpg", 0), ("mole/m.PNG", 1), ("zebra/a.png", 2), ("zebra/b.png", 2)]


def test_no_cpu_path():
    """Host features are refused: HipUnavailable without a device, ValueError with one."""
    with pytest.raises((hip.HipUnavailable, ValueError)):
        LP.ProbeObjective(torch.zeros(4, 64), torch.zeros(4, dtype=torch.long), 2, 0.1)
