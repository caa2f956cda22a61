"""msclip_rank_counts on the GPU against the numpy restatement (tests/metrics_ref.py), bitwise on the integers; its argument checks on
live device pointers; the drivers of msclip_amd/metrics.py against the committed scikit-learn values; and zeroshot.evaluate end to
end with the four TEST.METRIC values on generated VOC2007, Hateful Memes and ImageFolder sets."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import ROOT, synth_sd
from msclip_amd import evalsets, hip, linear_probe, metrics, metrics_hip, zeroshot
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p
FIXTURE = os.path.join(ROOT, "tests", "golden", "zeroshot_metrics_fixture.npz")


@functools.lru_cache(maxsize=None)
def _case(kind, N, C):
    """(S, Y, the restatement's counts): computed once per shape and kind, never written to."""
    S, Y = R.make_scores(kind, N, C, seed=N + C), R.make_labels(N, C, seed=N)
    return S, Y, R.counts(S, Y)


def _run(S, Y, lds, ldy, ldn, want_gt=True):
    """The kernel on windows of wider matrices; the outputs are prefilled with a sentinel."""
    N, C = S.shape
    dev = torch.device("cuda")
    Sw = torch.from_numpy(R.padded(S, lds, np.float32(np.nan))[0]).to(dev)
    Yw = torch.from_numpy(R.padded(Y, ldy, 1)[0]).to(dev)
    outs = tuple(torch.full((C, ldn), R.SENTINEL, dtype=torch.int32, device=dev) for _ in range(3))
    tot = tuple(torch.full((C,), R.SENTINEL, dtype=torch.int32, device=dev) for _ in range(2))
    metrics_hip.rank_counts(Sw[:, :C], Yw[:, :C], want_gt=want_gt, out=outs + tot)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], tot[0].cpu().numpy(), tot[1].cpu().numpy()


@pytest.mark.parametrize("N", R.EDGE_N)
def test_rank_counts_against_the_restatement(gpu_device, N):
    """Bitwise, at the edge sizes of the header's macros, C = 1 and 3 (a column of positives only and one of negatives only), lds > C,
    ldy > C, ldn > N with the slack untouched, every kind of score; two runs give the same bytes."""
    for C in (1, 3):
        for kind in R.KINDS:
            S, Y, want = _case(kind, N, C)
            outs, npos, nbad = _run(S, Y, C + 2, C + 5, N + 3)
            for got, ref, what in zip(outs, want[:3], ("ge_pos", "ge_neg", "gt_neg")):
                assert np.array_equal(got[:, :N], ref), (N, C, kind, what, np.argwhere(got[:, :N] != ref)[:5])
                assert (got[:, N:] == R.SENTINEL).all(), (N, C, kind, what)
            assert np.array_equal(npos, want[3]) and np.array_equal(nbad, want[4]) and not nbad.any(), (N, C, kind)
            if C == 3:
                assert npos[1] == N and npos[2] == 0
            if kind == "random":
                again = _run(S, Y, C + 2, C + 5, N + 3)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(outs + [npos, nbad], again[0] + [again[1], again[2]]))
    # gt_neg not asked for: the tensor in its slot of `out` is never written
    S, Y, want = _case("seven levels", N, 3)
    outs, npos, nbad = _run(S, Y, 3, 3, N, want_gt=False)
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1]) and (outs[2] == R.SENTINEL).all()


def test_rank_counts_column_view_and_nan(gpu_device):
    """S + 1 with C = 1 (what roc_auc reads), and NaN scores, which are counted in nbad."""
    N = R.ROWS + 37
    S, Y, _ = _case("random", N, 3)
    want = R.counts(S[:, 1:2], Y[:, 0:1])
    Sd, Yd = torch.from_numpy(S).cuda(), torch.from_numpy(np.ascontiguousarray(Y[:, 0:1])).cuda()
    got = metrics_hip.rank_counts(Sd[:, 1:2], Yd)
    assert Sd[:, 1:2].data_ptr() == Sd.data_ptr() + 4 and Sd[:, 1:2].stride(0) == 3
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    bad = S.copy()
    bad[::5, 0], bad[3, 2] = np.nan, np.nan
    _, _, _, npos, nbad = metrics_hip.rank_counts(torch.from_numpy(bad).cuda(), torch.from_numpy(Y).cuda())
    assert nbad.cpu().tolist() == [len(range(0, N, 5)), 0, 1] and np.array_equal(npos.cpu().numpy(), R.counts(S, Y)[3])
    with pytest.raises(ValueError, match="not a number"):
        metrics.average_precision_11(torch.from_numpy(bad).cuda(), Y)
    with pytest.raises(ValueError, match="not a number"):
        metrics.roc_auc(torch.from_numpy(bad).cuda(), (Y[:, 0] != 0).astype(np.int64), column=0)


def test_rank_counts_class_chunks(gpu_device, monkeypatch):
    """The binding's split of the class range (here with a small bound per launch) gives the counts of one launch."""
    N, C = 300, 5
    S, Y = R.make_scores("seven levels", N, C, seed=1), R.make_labels(N, C, seed=2)
    whole = metrics_hip.rank_counts(torch.from_numpy(S).cuda(), torch.from_numpy(Y).cuda())
    monkeypatch.setattr(metrics_hip, "LAUNCH_PAIRS", 2 * N * N)
    assert metrics_hip.class_chunks(N, C) == [(0, 2), (2, 2), (4, 1)]
    split = metrics_hip.rank_counts(torch.from_numpy(S).cuda(), torch.from_numpy(Y).cuda())
    for a, b, w in zip(whole, split, R.counts(S, Y)):
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), w)


def test_rank_counts_in_a_launch_plan(gpu_device):
    """The header's "recordable in a launch plan": the call recorded once (it runs while it is recorded) and replayed on other
    scores, handed in as the plan's external buffer, gives the counts of those scores."""
    N, C = R.STAGE + R.ROWS + 9, 3
    S1, S2, Y = R.make_scores("seven levels", N, C, seed=11), R.make_scores("random", N, C, seed=12), R.make_labels(N, C, seed=13)
    dev = torch.device("cuda")
    main = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(main):
        Sa, Sb, Yd = torch.from_numpy(S1).to(dev), torch.from_numpy(S2).to(dev), torch.from_numpy(Y).to(dev)
        out = metrics_hip.rank_counts(Sa, Yd)                                   # (allocates the outputs outside the recording)
        plan = hip.Plan(dev, [main])
        with plan.recording(externals=[Sa]):
            metrics_hip.rank_counts(Sa, Yd, out=out)
        assert plan.op_names() == ["msclip_rank_counts"]
        main.synchronize()
        for got, want in zip(out, R.counts(S1, Y)):
            assert np.array_equal(got.cpu().numpy(), want)
        for t in out:
            t.fill_(R.SENTINEL)
        plan.run([main], [Sb])
        main.synchronize()
    for got, want in zip(out, R.counts(S2, Y)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_rank_counts_rejected_arguments(gpu_device):
    """-1 and nothing launched (the outputs keep their sentinel): NULL and misaligned pointers, N = 0, lds < C, ldn < N, N * N * C
    over the bound.  Every pointer is a live allocation large enough for the accepted call."""
    L = metrics_hip.lib()
    hip.require_gpu()
    N, C = 16, 4
    dev = torch.device("cuda")
    S = torch.zeros(N + 1, 8, device=dev)
    Y = torch.zeros(N + 1, 8, dtype=torch.uint8, device=dev)
    outs = [torch.full((C + 1, N), R.SENTINEL, dtype=torch.int32, device=dev) for _ in range(3)]
    tot = [torch.full((C + 1,), R.SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
    ptr = dict(S=S.data_ptr(), Y=Y.data_ptr(), ge_pos=outs[0].data_ptr(), ge_neg=outs[1].data_ptr(), gt_neg=outs[2].data_ptr(),
               npos=tot[0].data_ptr(), nbad=tot[1].data_ptr())

    def rank(lds=8, ldy=8, N=N, C=C, ldn=N, **over):
        p = {k: (VP(v) if v else None) for k, v in dict(ptr, **over).items()}
        return L.msclip_rank_counts(p["S"], lds, p["Y"], ldy, N, C, p["ge_pos"], p["ge_neg"], p["gt_neg"], ldn, p["npos"], p["nbad"],
                                    hip._stream())
    for name in ("S", "Y", "ge_pos", "ge_neg", "npos", "nbad"):
        assert rank(**{name: 0}) == -1, name
    for name in ("S", "ge_pos", "ge_neg", "gt_neg", "npos", "nbad"):
        assert rank(**{name: ptr[name] + 2}) == -1 and rank(**{name: ptr[name] + 1}) == -1, name
    assert rank(N=0) == -1 and rank(C=0) == -1 and rank(lds=3) == -1 and rank(ldy=3) == -1 and rank(ldn=N - 1) == -1
    assert rank(N=2 ** 21, ldn=2 ** 21, C=2) == -1 and rank(N=2 ** 16, ldn=2 ** 16, C=2 ** 10 + 1, lds=2 ** 11, ldy=2 ** 11) == -1
    torch.cuda.synchronize()
    assert all(bool((t == R.SENTINEL).all()) for t in outs + tot)
    assert rank() == 0 and rank(gt_neg=0) == 0                                  # the accepted call
    torch.cuda.synchronize()
    assert bool((outs[0][:C] == 0).all()) and bool((outs[1][:C] == N).all()) and bool((outs[2][:C] == 0).all())
    assert tot[0].tolist() == [0] * C + [R.SENTINEL] and tot[1].tolist() == [0] * C + [R.SENTINEL]


def test_drivers_against_the_fixture(gpu_device):
    """The committed scikit-learn values (tools/make_metrics_fixture.py) through the device drivers, to 1e-12."""
    fx = np.load(FIXTURE)
    for k, name in enumerate(fx["names"]):
        s, y = fx[f"s{k}"], fx[f"y{k}"]
        S = torch.from_numpy(np.stack([-s, s], axis=1)).cuda()
        ap = metrics.average_precision_11(S[:, 1:2], y.reshape(-1, 1))[0]
        auc = metrics.roc_auc(S, y)
        print(f"{name}: ap11 {ap!r} ({abs(ap - fx['ap11'][k]):.3g}), auc {auc!r} ({abs(auc - fx['auc'][k]):.3g})")
        assert abs(ap - fx["ap11"][k]) <= 1e-12 and abs(auc - fx["auc"][k]) <= 1e-12, name
        assert abs(metrics.roc_auc(S, y, column=0) - (1.0 - fx["auc"][k])) <= 1e-12                # the mirrored column
    logits, y = torch.from_numpy(fx["mc_logits"]).cuda(), fx["mc_labels"]
    pred, rank = (torch.empty(len(y), dtype=torch.int32, device="cuda") for _ in range(2))
    metrics.predict_rows(logits, torch.from_numpy(y).to("cuda", torch.int32), pred, rank)
    assert np.array_equal(pred.cpu().numpy(), fx["mc_logits"].argmax(-1))                          # the lowest index on ties
    got = linear_probe.score_counts(pred, rank, y, logits.shape[1], "mean_per_class")["top1"]
    assert abs(got - 100.0 * float(fx["mc_balanced"])) <= 1e-10
    with pytest.raises(ValueError, match="Only one class present"):
        metrics.roc_auc(logits, np.ones(len(y), np.int64))


def test_drivers_against_the_restatement(gpu_device):
    """Several classes at once: exactly the formulas on the restatement's counts."""
    S, Y = R.make_scores("seven levels", 700, 5, seed=3), R.make_labels(700, 5, seed=4)
    ap, _ = R.formulas(S, Y)
    mean, per = metrics.average_precision_11(torch.from_numpy(S).cuda(), torch.from_numpy(Y))
    assert per == ap and mean == metrics.map11_percent(ap) / 100.0
    assert metrics.roc_auc(torch.from_numpy(S).cuda(), (Y[:, 0] != 0).astype(np.int64), column=0) == R.formulas(S, Y)[1][0]


# ---------------------------------------------------------------------------- evaluate, end to end
NAME = "b32-yfcc-msclips"
PROMPTS3 = (["aeroplane", "bus", "cat"], ["a photo of a {}.", "a {}."])


@pytest.fixture(scope="module")
def clip():
    from msclip_amd.tokenizer import SimpleTokenizer
    m = get_clip_model(named_config(NAME))                                      # random weights: plumbing
    m.load_state_dict(synth_sd(NAME), strict=True)
    return m.cuda().eval(), SimpleTokenizer()


def _jpegs(paths, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for p in paths:
        os.makedirs(os.path.dirname(p), exist_ok=True)
        low = rng.integers(0, 256, (5, 6, 3)).astype(np.uint8)
        Image.fromarray(np.repeat(np.repeat(low, 8, axis=0), 8, axis=1)).save(p, quality=90)


def _evaluate(clip, metric, classes, templates, **kw):
    lines = []
    res = zeroshot.evaluate(clip[0], clip[1], kw.pop("val_root", None), classes, templates, batch_size=8, metric=metric,
                            return_logits=True, log=lines.append, **kw)
    return res, lines


def test_evaluate_voc2007_map(gpu_device, clip, tmp_path):
    root = str(tmp_path) + os.sep
    base = os.path.join(root, *evalsets.VOC_SUFFIX["test"])
    os.makedirs(os.path.join(base, "ImageSets", "Main"))
    ids = [f"{i:06d}" for i in range(1, 25)]
    flags = np.random.RandomState(5).choice([" 1", " 0", "-1"], size=(3, 24), p=[0.4, 0.2, 0.4])
    for cat, row in zip(PROMPTS3[0], flags):
        with open(os.path.join(base, "ImageSets", "Main", f"{cat}_test.txt"), "w") as f:
            f.write("".join(f"{i} {flag}\n" for i, flag in zip(ids, row)))
    _jpegs([os.path.join(base, "JPEGImages", i + ".jpg") for i in ids], seed=1)
    items = evalsets.voc2007_items(root, "test")
    assert len(items) == 24 and np.array_equal(np.array([lab for _, lab in items]), (flags == " 1").T.astype(int))
    res, lines = _evaluate(clip, "11point_mAP", *PROMPTS3, items=items, dataset="voc2007classification")
    S, Y = res["logits"].numpy(), res["labels"].numpy()
    assert S.shape == (24, 3) and S.dtype == np.float32 and Y.shape == (24, 3) and res["n"] == 24 and res["top5"] is None
    assert res["top1"] == metrics.map11_percent(R.formulas(S, Y.astype(np.uint8))[0]) and 100.0 / 11 <= res["top1"] <= 100.0
    assert any(s.startswith("=> voc2007classification% TEST:") and "11point_mAP@1" in s for s in lines)
    with pytest.raises(ValueError, match="max_classes"):
        zeroshot.evaluate(clip[0], clip[1], None, *PROMPTS3, items=items, max_classes=2, metric="11point_mAP")


def test_evaluate_hatefulmemes_auc(gpu_device, clip, tmp_path):
    y = np.random.RandomState(6).randint(0, 2, size=24)
    y[:2] = (0, 1)
    with open(tmp_path / "dev_seen.jsonl", "w") as f:
        f.write("".join(json.dumps({"id": i, "img": f"img/{i:05d}.jpg", "label": int(v), "text": "t"}) + "\n" for i, v in enumerate(y)))
    items = evalsets.hatefulmemes_items(str(tmp_path), "val")
    _jpegs([p for p, _ in items], seed=2)
    res, lines = _evaluate(clip, "roc_auc", ["meme", "hatespeech meme"], ["a {}.", "this is a {}."], items=items, dataset="hatefulmemes")
    S = res["logits"].numpy()
    assert S.shape == (24, 2) and res["labels"].tolist() == y.tolist() and res["top5"] is None
    assert res["top1"] == R.formulas(S[:, 1:2], y.astype(np.uint8).reshape(-1, 1))[1][0] * 100 and 0.0 <= res["top1"] <= 100.0
    assert any(s.startswith("=> hatefulmemes% TEST:") and "roc_auc@1" in s for s in lines)


def test_evaluate_imagefolder_mean_per_class_and_accuracy(gpu_device, clip, tmp_path):
    counts = (12, 8, 4)                                                          # unbalanced: the two metrics differ
    paths = [str(tmp_path / "val" / f"n{c:03d}" / f"{k}.jpg") for c, n in enumerate(counts) for k in range(n)]
    _jpegs(paths, seed=3)
    root = str(tmp_path / "val")
    res, lines = _evaluate(clip, "mean-per-class", *PROMPTS3, val_root=root)
    S, y = res["logits"], res["labels"]
    assert S.shape == (24, 3) and y.tolist() == [0] * 12 + [1] * 8 + [2] * 4 and res["top5"] is None
    pred = torch.from_numpy(S.numpy().argmax(-1))                                # numpy's argmax: the lowest index on ties
    assert res["top1"] == metrics.mean_per_class(pred.numpy(), y.numpy(), 3) * 100
    assert abs(res["top1"] - linear_probe.score_counts(pred, torch.zeros_like(pred), y, 3, "mean_per_class")["top1"]) <= 1e-10
    assert any(s.startswith("=> imagenet% TEST:") and "mean-per-class@1" in s for s in lines)
    # accuracy: the keys and values of before this change
    acc, lines = _evaluate(clip, "accuracy", *PROMPTS3, val_root=root)
    assert set(acc) == {"top1", "top5", "n", "images_per_s", "elapsed_s", "loader_stats", "loader_threads", "loader_processes", "logits",
                        "classifier", "labels"}
    assert torch.equal(acc["logits"], S) and torch.equal(acc["labels"], y) and acc["n"] == 24
    a1, a5 = zeroshot.accuracy(acc["logits"], acc["labels"], (1, 3))
    assert abs(acc["top1"] - a1) <= 1e-9 and abs(acc["top5"] - a5) <= 1e-9 and acc["top5"] == 100.0
    assert any(s.startswith("=> imagenet% TEST:") and "accuracy@1" in s and "accuracy@5" in s for s in lines)
    with pytest.raises(ValueError, match="TEST.METRIC"):
        zeroshot.evaluate(clip[0], clip[1], root, *PROMPTS3, metric="f1")
    with pytest.raises(ValueError, match="not both"):
        zeroshot.evaluate(clip[0], clip[1], root, *PROMPTS3, items=[(paths[0], 0)])
