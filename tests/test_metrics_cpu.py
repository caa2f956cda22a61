"""The zero-shot metrics without a GPU: include/msclip_metrics.h as msclip_amd/metrics_hip.py binds it, msclip_rank_counts' argument
validation (host side, before any launch), the counting built for the host (tests/metrics_host.cpp) against the numpy restatement
(tests/metrics_ref.py), the formulas of msclip_amd/metrics.py against scikit-learn and against the committed fixture, the dataset
readers, load_prompts by name, and evaluate's arguments."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import ROOT
from msclip_amd import abi, color_hip, evalsets, hip, input_hip, metrics, metrics_hip, zeroshot

VP, CI = ctypes.c_void_p, ctypes.c_int
TOL = 1e-12                       # integer sums are exact in double, one division is one ulp; scikit-learn's trapezoid accumulates
#                                   at most about N * 2^-53 = 1.2e-13 at N = 1100
FIXTURE = os.path.join(ROOT, "tests", "golden", "zeroshot_metrics_fixture.npz")
CASES = R.metric_cases()


def _build():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()


# ---------------------------------------------------------------------------- the header and its binding
def test_metrics_header_binding():
    met = abi.load(metrics_hip.HEADER, metrics_hip.VERSION_MACRO)
    assert os.path.basename(metrics_hip.HEADER) == "msclip_metrics.h" and met.version == 1 == metrics_hip.METRICS_ABI_VERSION
    assert not met.structs
    assert met.protos == {
        "msclip_rank_counts": (CI, [VP, CI, VP, CI, CI, CI, VP, VP, VP, CI, VP, VP, VP]),
        "msclip_metrics_abi_version": (CI, []),
    }
    assert metrics_hip.METRICS_EXPORTS == tuple(met.protos)
    main = abi.load()
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    ext4 = abi.load(abi.EXT4_HEADER, abi.EXT4_VERSION_MACRO, known=tuple(main.structs) + tuple(ext3.structs))
    ext5 = abi.load(abi.EXT5_HEADER, abi.EXT5_VERSION_MACRO)
    inp = abi.load(input_hip.HEADER, input_hip.VERSION_MACRO)
    col = abi.load(color_hip.HEADER, color_hip.VERSION_MACRO)
    for older in (main, ext, ext2, ext3, ext4, ext5, inp, col):
        assert not set(met.protos) & set(older.protos)
    assert [row[0] for row in hip._BOUND] == ["_ABI", "_EXT", "_EXT2", "_EXT3", "_EXT4", "_EXT5"]
    assert (metrics_hip.RANK_ROWS, metrics_hip.RANK_STAGE) == (R.ROWS, R.STAGE) == (256, 1024) and metrics_hip.MAX_PAIRS == 2 ** 42
    _build()
    L = metrics_hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in metrics_hip.METRICS_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_metrics_abi_version() == 1


def test_rank_counts_rejections():
    """Every MSCLIP_EINVAL rule on fake non-null pointers: a call that got past its checks would launch on them."""
    _build()
    L = metrics_hip.lib()
    p, odd, two = VP(0x10000), VP(0x10001), VP(0x10002)

    def rank(S=p, lds=8, Y=p, ldy=8, N=16, C=4, ge_pos=p, ge_neg=p, gt_neg=p, ldn=16, npos=p, nbad=p):
        return L.msclip_rank_counts(S, lds, Y, ldy, N, C, ge_pos, ge_neg, gt_neg, ldn, npos, nbad, None)
    for name in ("S", "Y", "ge_pos", "ge_neg", "npos", "nbad"):
        assert rank(**{name: None}) == -1, name                              # null
    for name in ("S", "ge_pos", "ge_neg", "gt_neg", "npos", "nbad"):
        assert rank(**{name: two}) == -1 and rank(**{name: odd}) == -1, name # misaligned
    assert rank(N=0) == -1 and rank(N=-5) == -1 and rank(C=0) == -1 and rank(C=-1) == -1
    assert rank(lds=3) == -1 and rank(ldy=3) == -1 and rank(ldn=15) == -1
    assert rank(N=2 ** 21, ldn=2 ** 21, C=2, lds=2, ldy=2) == -1              # 2^43 comparisons
    assert rank(N=2 ** 21 + 1, ldn=2 ** 21 + 1, C=1, lds=1, ldy=1) == -1
    assert rank(N=2 ** 16, ldn=2 ** 16, C=2 ** 10 + 1, lds=2 ** 11, ldy=2 ** 11) == -1
    assert rank(N=2 ** 31 - 1, ldn=2 ** 31 - 1, C=1) == -1


def test_class_chunks():
    """The binding cuts the class range so that a launch compares at most 2^40 pairs."""
    assert metrics_hip.class_chunks(4952, 20) == [(0, 20)]
    assert metrics_hip.class_chunks(2 ** 19, 10) == [(0, 4), (4, 4), (8, 2)]
    assert metrics_hip.class_chunks(2 ** 20, 3) == [(0, 1), (1, 1), (2, 1)]
    for N, C in ((50000, 1000), (2 ** 19 + 1, 7)):
        ch = metrics_hip.class_chunks(N, C)
        assert all(N * N * cols <= 2 ** 40 for _, cols in ch) and [c0 for c0, _ in ch] == list(np.cumsum([0] + [c for _, c in ch])[:-1])
        assert sum(cols for _, cols in ch) == C
    with pytest.raises(ValueError, match="comparisons per class"):
        metrics_hip.class_chunks(2 ** 20 + 1, 1)


# ---------------------------------------------------------------------------- the counting on the host
def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, g++, or the clang++ that hipcc drives)"
    return cxx


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/metrics_host.cpp (the counting, msclip_amd/csrc/rank_body.h) built with metrics.hip's floating-point flags."""
    so = str(tmp_path_factory.mktemp("metrics_host") / "libmetrics_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "metrics_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def test_host_program_under_sanitizers(tmp_path):
    """tests/metrics_host.cpp as a stand-alone program under AddressSanitizer and UBSan: ragged shapes, NaN / +-Inf scores, label
    bytes 0 / 1 / 255, matrices that end with their last row, LDS buffers of exactly the device's size."""
    exe = str(tmp_path / "metrics_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DMETRICS_HOST_MAIN",
                    os.path.join(ROOT, "tests", "metrics_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "metrics_host: checksum" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _host(L, S, Y, lds, ldy, ldn, want_gt=True):
    N, C = S.shape
    Sw, _ = R.padded(S, lds, np.float32(np.nan))
    Yw, _ = R.padded(Y, ldy, 1)
    outs = [np.full((C, ldn), R.SENTINEL, np.int32) for _ in range(3)]
    npos, nbad = np.full(C, R.SENTINEL, np.int32), np.full(C, R.SENTINEL, np.int32)
    P = lambda a: a.ctypes.data_as(VP)                                # noqa: E731
    assert L.host_rank_counts(P(Sw), lds, P(Yw), ldy, N, C, P(outs[0]), P(outs[1]), P(outs[2]) if want_gt else None, ldn, P(npos),
                              P(nbad)) == 0
    return outs, npos, nbad


@pytest.mark.parametrize("N", R.EDGE_N)
def test_host_build_of_the_counting(host_lib, N):
    """Exactly the restatement, at the edge sizes of the header's macros, C = 1 and 3, every kind of score, leading dimensions with
    slack that comes back untouched."""
    assert (host_lib.host_rank_rows(), host_lib.host_rank_stage()) == (R.ROWS, R.STAGE)
    for C in (1, 3):
        Y = R.make_labels(N, C, seed=N)
        for kind in R.KINDS:
            S = R.make_scores(kind, N, C, seed=N + C)
            want = R.counts(S, Y)
            outs, npos, nbad = _host(host_lib, S, Y, C + 2, C + 5, N + 3)
            for got, ref, what in zip(outs, want[:3], ("ge_pos", "ge_neg", "gt_neg")):
                assert np.array_equal(got[:, :N], ref), (N, C, kind, what)
                assert (got[:, N:] == R.SENTINEL).all(), (N, C, kind, what)
            assert np.array_equal(npos, want[3]) and np.array_equal(nbad, want[4]) and not nbad.any()
    # without gt_neg; NaN scores: counted in nbad, compared false both ways
    S, Y = R.make_scores("random", N, 3, seed=5), R.make_labels(N, 3, seed=6)
    S[::3, 0] = np.nan
    want = R.counts(S, Y)
    outs, npos, nbad = _host(host_lib, S, Y, 3, 3, N, want_gt=False)
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1]) and (outs[2] == R.SENTINEL).all()
    assert np.array_equal(nbad, want[4]) and nbad[0] == len(range(0, N, 3)) and np.array_equal(npos, want[3])


def test_restatement_properties():
    """The restatement against first principles on a column small enough to read."""
    S = np.array([[0.5], [0.5], [-0.0], [0.0], [np.inf], [-np.inf], [2.0]], np.float32)
    Y = np.array([[1], [0], [1], [0], [0], [1], [255]], np.uint8)
    ge_pos, ge_neg, gt_neg, npos, nbad = R.counts(S, Y)
    assert ge_pos[0].tolist() == [2, 2, 3, 3, 0, 4, 1] and ge_neg[0].tolist() == [2, 2, 3, 3, 1, 3, 1]
    assert gt_neg[0].tolist() == [1, 1, 2, 2, 0, 3, 1] and npos[0] == 4 and nbad[0] == 0


# ---------------------------------------------------------------------------- the formulas
def _one(s, y):
    S, Y = s.reshape(-1, 1), y.reshape(-1, 1)
    ap, auc = R.formulas(S, Y)
    return ap[0], auc[0]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_formulas_against_scikit_learn(case):
    pytest.importorskip("sklearn")
    from sklearn.metrics import roc_auc_score
    _, s, y = case
    ap, auc = _one(s, y)
    want_ap, want_auc = R.sklearn_map11(y, s), roc_auc_score(y, s)
    print(f"{case[0]}: ap11 {ap!r} vs {want_ap!r} ({abs(ap - want_ap):.3g}), auc {auc!r} vs {want_auc!r} ({abs(auc - want_auc):.3g})")
    assert abs(ap - want_ap) <= TOL and abs(auc - want_auc) <= TOL


def test_mean_per_class_against_scikit_learn():
    pytest.importorskip("sklearn")
    from sklearn.metrics import balanced_accuracy_score
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_metrics_fixture as F
    logits, y = F.multiclass_case()
    assert 5 not in y                                                         # a class absent from the labels does not count
    got = metrics.mean_per_class(logits.argmax(-1), y, 7)
    assert abs(got - balanced_accuracy_score(y, logits.argmax(-1))) <= TOL
    r = np.random.RandomState(3)
    for C in (2, 10):
        y, pred = r.randint(0, C, size=500), r.randint(0, C, size=500)
        assert abs(metrics.mean_per_class(pred, y, C) - balanced_accuracy_score(y, pred)) <= TOL


def test_formulas_against_the_fixture():
    """The committed scikit-learn values (tools/make_metrics_fixture.py): the same check where scikit-learn is absent."""
    fx = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 64 * 1024 and [str(n) for n in fx["names"]] == [c[0] for c in CASES]
    for k, (name, s, y) in enumerate(CASES):
        assert np.array_equal(fx[f"s{k}"], s) and np.array_equal(fx[f"y{k}"], y), name      # the fixture holds metric_cases' data
        ap, auc = _one(fx[f"s{k}"], fx[f"y{k}"])
        assert abs(ap - fx["ap11"][k]) <= TOL and abs(auc - fx["auc"][k]) <= TOL, name
    logits, y = fx["mc_logits"], fx["mc_labels"]
    assert abs(metrics.mean_per_class(logits.argmax(-1), y, logits.shape[1]) - float(fx["mc_balanced"])) <= TOL


def test_ap11_by_hand():
    """Scores 4 3 2 1 with labels + - + -: precision / recall points (1, .5) (.5, .5) (2/3, 1) (.5, 1).  Levels 1.0 ... 0.6 see
    2/3, levels 0.5 ... 0.1 see 1, level 0 gives 1."""
    s, y = np.array([4, 3, 2, 1], np.float32), np.array([1, 0, 1, 0], np.uint8)
    ap, auc = _one(s, y)
    assert abs(ap - (5 * (2 / 3) + 5 * 1 + 1) / 11) <= 1e-14 and auc == 0.75
    assert metrics.RECALL_THRESHOLDS == np.linspace(1, 0, 11).tolist() and metrics.RECALL_THRESHOLDS[-1] == 0.0
    # no positive: scikit-learn sets the recall to one, every precision is zero, the appended point gives the level 0 its 1.0
    assert metrics.ap11_from_counts([0, 0, 0], [1, 2, 3], 0) == 1.0 / 11
    assert metrics.map11_percent([0.5, 0.25]) == 37.5


def test_error_cases():
    s, y = np.array([1, 2, 3], np.float32).reshape(-1, 1), np.array([1, 1, 1], np.uint8).reshape(-1, 1)
    ge_pos, ge_neg, gt_neg, npos, nbad = R.counts(s, y)
    with pytest.raises(ValueError, match="Only one class present"):
        metrics.auc_from_counts(ge_neg[0], gt_neg[0], y[:, 0] != 0, nbad[0])
    with pytest.raises(ValueError, match="Only one class present"):
        metrics.auc_from_counts(ge_neg[0], gt_neg[0], np.zeros(3, bool), nbad[0])
    s[1, 0], y[0, 0] = np.nan, 0
    ge_pos, ge_neg, gt_neg, npos, nbad = R.counts(s, y)
    assert nbad[0] == 1
    with pytest.raises(ValueError, match="not a number"):
        metrics.auc_from_counts(ge_neg[0], gt_neg[0], y[:, 0] != 0, nbad[0])
    with pytest.raises(ValueError, match="not a number"):
        metrics.ap11_from_counts(ge_pos[0], ge_neg[0], npos[0], nbad[0])
    # mean-per-class with a class absent from the labels: classes 0 and 2 occur, recalls 1/2 and 1
    assert metrics.mean_per_class([0, 1, 2], [0, 0, 2], 3) == 0.75


# ---------------------------------------------------------------------------- readers and prompts
def _voc_tree(root, image_set="test"):
    base = os.path.join(root, *evalsets.VOC_SUFFIX[image_set])
    os.makedirs(os.path.join(base, "ImageSets", "Main"))
    os.makedirs(os.path.join(base, "JPEGImages"))
    rows = {"cat": [("000003", " 1"), ("000001", "-1"), ("000002", " 0"), ("000010", " 1")],
            "aeroplane": [("000001", " 1"), ("000002", "-1"), ("000003", " 1"), ("000010", "-1")],
            "bus": [("000001", "-1"), ("000002", "-1"), ("000003", " 0"), ("000010", " 1"), ("000007", " 1")]}   # 000007: here only
    for cat, lines in rows.items():
        with open(os.path.join(base, "ImageSets", "Main", f"{cat}_{image_set}.txt"), "w") as f:
            f.write("".join(f"{i} {flag}\n" for i, flag in lines))
    for other in ("cat_trainval.txt", image_set + ".txt"):                    # not category files of this set
        with open(os.path.join(base, "ImageSets", "Main", other), "w") as f:
            f.write("000099  1\n")
    return base


def test_voc2007_reader(tmp_path):
    root = str(tmp_path) + os.sep
    base = _voc_tree(root)
    assert evalsets.voc2007_categories(root, "test") == ["aeroplane", "bus", "cat"]
    items = evalsets.voc2007_items(root, "test")
    assert [os.path.relpath(p, base) for p, _ in items] == [os.path.join("JPEGImages", f"{i}.jpg") for i in
                                                            ("000001", "000002", "000003", "000007", "000010")]
    assert [lab for _, lab in items] == [[1, 0, 0], [0, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1]]
    assert base.endswith(os.path.join("test", "VOCdevkit 2", "VOC2007"))
    _voc_tree(root, "val")
    assert evalsets.voc2007_items(root, "val")[0][0].startswith(os.path.join(root, "train", "VOCdevkit", "VOC2007"))
    with pytest.raises(ValueError, match="Incorrect image set"):
        evalsets.voc2007_items(root, "dev")


def test_hatefulmemes_reader(tmp_path):
    recs = [{"id": 1, "img": "img/00001.png", "label": 1, "text": "a"}, {"id": 2, "img": "img/00002.png", "label": 0, "text": "b"}]
    with open(tmp_path / "dev_seen.jsonl", "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in recs))
    with open(tmp_path / "train.jsonl", "w") as f:
        f.write(json.dumps(recs[1]) + "\n")
    root = str(tmp_path)
    assert evalsets.hatefulmemes_items(root, "val") == [(os.path.join(root, "img/00001.png"), 1), (os.path.join(root, "img/00002.png"), 0)]
    assert evalsets.hatefulmemes_items(root, "train") == [(os.path.join(root, "img/00002.png"), 0)]
    with pytest.raises(ValueError, match="Incorrect image_set"):
        evalsets.hatefulmemes_items(root, "test")


def test_load_prompts_by_name(tmp_path):
    imagenet = zeroshot.load_prompts("imagenet")
    assert len(imagenet[0]) == 1000 and len(imagenet[1]) == 80
    assert zeroshot.load_prompts(zeroshot.PROMPTS["imagenet"]) == imagenet                       # today's calls, unchanged
    voc = {"classes": ["aeroplane", "bus", "cat"], "templates": ["a photo of a {}.", "a {}."]}
    named, flat = str(tmp_path / "named.json"), str(tmp_path / "flat.json")
    with open(named, "w") as f:
        json.dump({"voc2007classification": voc, "imagenet": {"classes": ["tench"], "templates": ["{}"]}}, f)
    with open(flat, "w") as f:
        json.dump(voc, f)
    assert zeroshot.load_prompts(named, "voc2007classification") == (voc["classes"], voc["templates"])
    assert zeroshot.load_prompts(named) == (["tench"], ["{}"])
    assert zeroshot.load_prompts(flat) == zeroshot.load_prompts(flat, "voc2007classification") == (voc["classes"], voc["templates"])
    with pytest.raises(ValueError, match="Can not find prompt"):
        zeroshot.load_prompts(named, "hatefulmemes")
    const, old = str(tmp_path / "constants.py"), str(tmp_path / "old_constants.py")
    with open(const, "w") as f:
        f.write("ALL_CLASSES_DICT = {'imagenet': ['tench'], 'hatefulmemes': ['meme', 'hatespeech meme']}\n"
                "ALL_TEMPLATES_DICT = {'imagenet': ['{}'], 'hatefulmemes': ['a {}.', lambda c: f'this is a {c}.']}\n")
    with open(old, "w") as f:
        f.write("IMAGENET_CLASSES = ['goldfish']\nIMAGENET_DEFAULT_TEMPLATES = ['a photo of a {}.']\n")
    assert zeroshot.load_prompts(const, "hatefulmemes") == (["meme", "hatespeech meme"], ["a {}.", "this is a {}."])
    assert zeroshot.load_prompts(const) == (["tench"], ["{}"])
    assert zeroshot.load_prompts(old) == (["goldfish"], ["a photo of a {}."])
    with pytest.raises(ValueError, match="Can not find prompt"):
        zeroshot.load_prompts(old, "hatefulmemes")


def test_eval_cli_datasets():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_zeroshot as E
    model = os.path.join(ROOT, "experiments/model/b32-yfcc-msclips.yaml")
    for name, metric in (("voc2007classification", "11point_mAP"), ("hatefulmemes", "roc_auc"), ("imagenet", "accuracy")):
        c = E.build_config(E.resolve_dataset(name), model, ["DATASET.ROOT", "/data/x/"])
        assert c.DATASET.DATASET == name and c.TEST.METRIC == metric and c.DATASET.ROOT == "/data/x/"
        assert (name in E.READERS) == (name != "imagenet")
    assert list(E.cfg_files_dataset) == ["imagenet"]                          # the loop of a run without --ds
    a = E.parse_args(["--model", model, "--ds", "hatefulmemes", "--prompts", "p.json"])
    assert a.prompts == "p.json" and E.parse_args(["--model", model]).prompts is None


def test_evaluate_arguments():
    """The three metrics get as far as the GPU: HipUnavailable here, where evaluate used to raise NotImplementedError first."""
    assert zeroshot.METRICS == ("accuracy", "mean-per-class", "11point_mAP", "roc_auc")
    if not torch.cuda.is_available():                     # (with a GPU tests/test_gpu_metrics.py runs evaluate end to end)
        for metric in zeroshot.METRICS[1:]:
            with pytest.raises(hip.HipUnavailable):
                zeroshot.evaluate(None, None, "/nonexistent", ["a", "b"], ["{}"], metric=metric)
    items = [("a.jpg", [1, 0]), ("b.jpg", [0, 1])]
    with pytest.raises(ValueError, match="multi-hot label row of 3"):
        zeroshot._check_items(items, "11point_mAP", 3)
    with pytest.raises(ValueError, match="one class index per image"):
        zeroshot._check_items(items, "roc_auc", 2)
    with pytest.raises(ValueError, match="outside"):
        zeroshot._check_items([("a.jpg", 2)], "mean-per-class", 2)
    zeroshot._check_items(items, "11point_mAP", 2)
    zeroshot._check_items([("a.jpg", 1), ("b.jpg", 0)], "roc_auc", 2)
