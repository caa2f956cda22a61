"""TRAIN.OPTIMIZER lamb without a GPU: the fp64 restatement (tests/lamb_ref.py) against torch's own optimizer and on the edge
rules, the config reader, the LAMB extension header's binding and struct layout, the host batcher with the LAMB item, and the
checkpoint's optimizer block."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import lamb_ref as R
from conftest import ROOT
from msclip_amd import abi, hip, train
from msclip_amd.config import named_config

B32 = "b32-yfcc-msclips"
VP, CI, CF, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
F64 = torch.float64


def _tensors(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = {"a.weight": (7, 5), "a.bias": (7,), "b.weight": (33,), "scalar": ()}
    return ({k: torch.randn(s, generator=g, dtype=F64) * (0.5 + i) for i, (k, s) in enumerate(shapes.items())},
            [{k: torch.randn(s, generator=g, dtype=F64) * 0.1 for k, s in shapes.items()} for _ in range(3)])


# ---------------------------------------------------------------------------- the restatement
def test_reference_without_decay_is_torch_adamw():
    """Every wd = 0 and always_adapt off: no tensor adapts, LAMB is Adam -- three steps against torch.optim.AdamW in fp64."""
    params, grads = _tensors()
    mine = {k: v.clone() for k, v in params.items()}
    theirs = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
    opt = torch.optim.AdamW(list(theirs.values()), lr=3e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0)
    state = {}
    for t, g in enumerate(grads, 1):
        out = R.lamb_step(mine, g, state, t, 3e-3, 0.0, betas=(0.9, 0.98), eps=1e-6)
        mine = {k: o["w"] for k, o in out.items()}
        for k, p in theirs.items():
            p.grad = g[k].clone()
        opt.step()
        for k in mine:
            assert float(out[k]["r"]) == 1.0
            assert float((mine[k] - theirs[k].detach()).abs().max()) <= 1e-12, (t, k)


def test_reference_step_length_is_lr_times_the_weight_norm():
    params, grads = _tensors(1)
    wd = {"a.weight": 0.2, "a.bias": 0.0, "b.weight": 0.05, "scalar": 0.1}
    state = {}
    for t, g in enumerate(grads, 1):
        out = R.lamb_step(params, g, state, t, 1e-2, wd)
        for k, o in out.items():
            step, wn = float(torch.linalg.vector_norm(o["delta"])), float(torch.linalg.vector_norm(params[k]))
            if wd[k]:
                assert abs(step - 1e-2 * wn) <= 1e-12 * wn, (t, k)
                assert abs(float(o["r"]) - float(o["wn"] / o["un"])) <= 1e-15
            else:
                assert float(o["r"]) == 1.0 and torch.equal(o["delta"], -1e-2 * o["u"])
        params = {k: o["w"] for k, o in out.items()}
    always = R.lamb_step(params, grads[0], {}, 1, 1e-2, wd, always_adapt=True)["a.bias"]
    assert float(always["r"]) == float(always["wn"] / always["un"]) != 1.0


def test_reference_edge_rules():
    w = {"z": torch.zeros(5, dtype=F64), "u0": torch.ones(4, dtype=F64), "nan": torch.ones(6, dtype=F64), "big": torch.full((3,), 10.0, dtype=F64)}
    g = {"z": torch.ones(5, dtype=F64), "u0": torch.zeros(4, dtype=F64), "nan": torch.ones(6, dtype=F64), "big": torch.full((3,), 1e-3, dtype=F64)}
    g["nan"][2] = float("nan")
    wd = {"z": 0.1, "u0": 0.0, "nan": 0.1, "big": 0.0}
    out = R.lamb_step(w, g, {}, 1, 1e-2, wd, always_adapt=True)
    assert float(out["z"]["r"]) == 1.0 and float(out["z"]["wn"]) == 0.0 and float(out["z"]["un"]) > 0      # all-zero weight
    assert float(out["u0"]["r"]) == 1.0 and float(out["u0"]["un"]) == 0.0 and torch.equal(out["u0"]["w"], w["u0"])   # u = 0
    bad = torch.isnan(out["nan"]["w"])
    assert float(out["nan"]["r"]) == 1.0 and bad.tolist() == [False, False, True, False, False, False]     # NaN only where u is NaN
    assert torch.equal(torch.isnan(out["nan"]["u"]), bad)
    assert float(out["big"]["r"]) > 1.0                                                                      # ||w|| = 17.3, ||u|| = 1.7
    capped = R.lamb_step(w, g, {}, 1, 1e-2, wd, always_adapt=True, trust_clip=True)
    assert float(capped["big"]["r"]) == 1.0 and float(capped["z"]["r"]) == 1.0
    small = R.lamb_step({"s": torch.full((3,), 0.01, dtype=F64)}, {"s": torch.ones(3, dtype=F64)}, {}, 1, 1e-2, 0.1, trust_clip=True)["s"]
    assert float(small["r"]) == float(small["wn"] / small["un"]) < 1.0                                      # below 1: untouched


# ---------------------------------------------------------------------------- config
def test_lamb_settings_from_the_config():
    adamw = dict(lr=0.0001, lr_share=0.0001, wd=0.05, wd_share=0.2, betas=(0.9, 0.999), eps=1e-8, without_wd=("bn", "bias", "ln"))
    assert train.optimizer_settings(named_config(B32)) == adamw                          # adamW: what it was
    lamb = dict(adamw, eps=1e-6, optimizer="lamb", trust_clip=False, always_adapt=False, clip_grad_norm=0.0)
    for spelling in ("lamb", "LAMB", "Lamb"):
        assert train.optimizer_settings(named_config(B32, ["TRAIN.OPTIMIZER", spelling])) == lamb
    timm = ["TRAIN.OPTIMIZER", "timm", "TRAIN.OPTIMIZER_ARGS.opt", "lamb"]
    assert train.optimizer_settings(named_config(B32, timm)) == lamb
    full = train.optimizer_settings(named_config(B32, timm + [
        "TRAIN.OPTIMIZER_ARGS.opt_betas", "[0.9, 0.98]", "TRAIN.OPTIMIZER_ARGS.opt_eps", "1e-7", "TRAIN.OPTIMIZER_ARGS.trust_clip", "True",
        "TRAIN.OPTIMIZER_ARGS.always_adapt", "True", "TRAIN.OPTIMIZER_ARGS.bias_correction", "True",
        "TRAIN.OPTIMIZER_ARGS.grad_averaging", "True", "TRAIN.OPTIMIZER_ARGS.lr", "0.5", "TRAIN.OPTIMIZER_ARGS.max_grad_norm", "2.0"]))
    assert full == dict(lamb, betas=(0.9, 0.98), eps=1e-7, trust_clip=True, always_adapt=True, clip_grad_norm=2.0)
    lam = ["TRAIN.OPTIMIZER", "lamb"]
    assert train.optimizer_settings(named_config(B32, lam + ["TRAIN.OPTIMIZER_ARGS.betas", "[0.8, 0.9]", "TRAIN.OPTIMIZER_ARGS.eps", "1e-5"])) \
        == dict(lamb, betas=(0.8, 0.9), eps=1e-5)
    # max_grad_norm <-> CLIP_GRAD_NORM
    assert train.optimizer_settings(named_config(B32, lam + ["TRAIN.CLIP_GRAD_NORM", "1.5"]))["clip_grad_norm"] == 1.5
    both = lam + ["TRAIN.CLIP_GRAD_NORM", "1.5", "TRAIN.OPTIMIZER_ARGS.max_grad_norm"]
    assert train.optimizer_settings(named_config(B32, both + ["1.5"]))["clip_grad_norm"] == 1.5
    with pytest.raises(ValueError, match="max_grad_norm"):
        train.optimizer_settings(named_config(B32, both + ["1.0"]))
    # what is not implemented raises
    for extra in (["TRAIN.OPTIMIZER_ARGS.bias_correction", "False"], ["TRAIN.OPTIMIZER_ARGS.grad_averaging", "False"],
                  ["TRAIN.OPTIMIZER_ARGS.momentum", "0.9"]):
        with pytest.raises(NotImplementedError):
            train.optimizer_settings(named_config(B32, lam + extra))
    for other in (["TRAIN.OPTIMIZER", "timm", "TRAIN.OPTIMIZER_ARGS.opt", "lars"], ["TRAIN.OPTIMIZER", "timm"], ["TRAIN.OPTIMIZER", "sgd"]):
        with pytest.raises(NotImplementedError):
            train.optimizer_settings(named_config(B32, other))
    with pytest.raises(NotImplementedError):                                             # adamW does not grow LAMB's keys
        train.optimizer_settings(named_config(B32, ["TRAIN.OPTIMIZER_ARGS.trust_clip", "True"]))
    assert train.OPTIMIZERS == {"adamw": 1e-8, "lamb": 1e-6}


# ---------------------------------------------------------------------------- the extension header
_LAMB_FIELDS = ["p", "g", "m", "v", "n", "lr", "weight_decay", "pk", "pk_scale", "pk_f32", "param", "adapt"]


def test_lamb_header_binding():
    main = abi.load()
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    assert os.path.basename(abi.EXT3_HEADER) == "msclip_ext3.h" and ext3.version == 1 == hip.EXT3_ABI_VERSION
    assert list(ext3.structs) == ["msclip_lamb_tensor"] and hip.LambTensor is hip._EXT3.structs["msclip_lamb_tensor"]
    assert ext3.protos == {
        "msclip_lamb_partials": (CI, [VP, CI, CF, CF, CF, CI, VP, VP, LL, VP]),
        "msclip_lamb_ratios": (CI, [VP, VP, CI, LL, CI, VP, VP]),
        "msclip_lamb_apply": (CI, [VP, CI, CF, CF, CF, CI, VP, VP, VP]),
        "msclip_ext3_abi_version": (CI, []),
    }
    assert hip.EXT3_EXPORTS == tuple(ext3.protos)
    assert not set(ext3.protos) & (set(main.protos) | set(hip.EXT_EXPORTS) | set(hip.EXT2_EXPORTS))
    # msclip_adamw_tensor's members in its order, then the two new ones
    assert [f for f, _ in hip.LambTensor._fields_] == _LAMB_FIELDS
    assert hip.LambTensor._fields_[:10] == hip.AdamwTensor._fields_ and hip.LambTensor._fields_[10:] == [("param", CI), ("adapt", CI)]
    # the older headers are what they were
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    assert main.version == 9 and len(main.protos) == 107 and ext.version == 1 and ext2.version == 1
    assert len(ext.protos) == 2 and len(ext2.protos) == 4 and ctypes.sizeof(hip.AdamwTensor) == 64


def test_lamb_tensor_layout_matches_the_c_compilers(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "msclip_ext3.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(msclip_lamb_tensor));']
    expect = [f"size {ctypes.sizeof(hip.LambTensor)}"]
    for field in _LAMB_FIELDS:
        lines.append(f'  printf("{field} %zu\\n", offsetof(msclip_lamb_tensor, {field}));')
        expect.append(f"{field} {getattr(hip.LambTensor, field).offset}")
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    cc = shutil.which("cc") or "/opt/rocm/lib/llvm/bin/clang"
    assert os.path.exists(cc), "no host C compiler (cc, or the clang that hipcc drives)"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"),
                    "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert got == expect
    assert got[0] == "size 72" and "param 64" in got and "adapt 68" in got


def test_library_exports_the_lamb_entry_points():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.EXT3_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_ext3_abi_version() == 1
    # rejected before anything launches (fake non-null pointers)
    p = ctypes.c_void_p(0x10000)
    arr = (hip.LambTensor * 2)()
    for a, n, k in zip(arr, (5, 40000), (0, 1)):
        a.p = a.g = a.m = a.v = 0x10000
        a.n, a.lr, a.param, a.adapt = n, 1e-3, k, 1
    args = (0.9, 0.999, 1e-6, 1)
    assert L.msclip_lamb_partials(None, 2, *args, None, p, 6, None) == -1
    assert L.msclip_lamb_partials(arr, 2, *args, None, None, 6, None) == -1
    for wrong in (0, 3, 5, 7):                                             # 1 + 2 chunks: six partials, nothing else
        assert L.msclip_lamb_partials(arr, 2, *args, None, p, wrong, None) == -1
    assert L.msclip_lamb_partials(arr, 2, 0.9, 0.999, 1e-6, 0, None, p, 6, None) == -1          # step < 1
    assert L.msclip_lamb_apply(None, 2, *args, None, p, None) == -1
    assert L.msclip_lamb_apply(arr, 2, *args, None, None, None) == -1
    arr[1].param = 2                                                       # parameters are numbered without gaps
    assert L.msclip_lamb_partials(arr, 2, *args, None, p, 6, None) == -1 and L.msclip_lamb_apply(arr, 2, *args, None, p, None) == -1
    arr[1].param, arr[0].p = 1, None
    assert L.msclip_lamb_partials(arr, 2, *args, None, p, 6, None) == -1 and L.msclip_lamb_apply(arr, 2, *args, None, p, None) == -1
    assert L.msclip_lamb_ratios(None, p, 2, 3, 0, p, None) == -1
    assert L.msclip_lamb_ratios(p, None, 2, 3, 0, p, None) == -1
    assert L.msclip_lamb_ratios(p, p, 2, 3, 0, None, None) == -1
    assert L.msclip_lamb_ratios(p, p, 0, 3, 0, p, None) == -1


# ---------------------------------------------------------------------------- the host batcher with the LAMB item
_BATCH_PROGRAM = r"""
#include <stdio.h>
#include "multi_tensor.h"
#include "msclip_ext3.h"
using Batch = MtBatch<msclip_lamb_tensor, NT_, NB_>;
int main(void) {
  static msclip_lamb_tensor items[128];
  int count = 0;
  long long n;
  while (count < 128 && scanf("%lld", &n) == 1) {
    msclip_lamb_tensor& t = items[count];
    t.p = t.m = t.v = (float*)((unsigned long long)count << 34);      // element index count << 32
    t.g = t.p;
    t.n = n;
    t.param = count / 2;
    t.adapt = count & 1;
    ++count;
  }
  printf("sizeof %zu\n", sizeof(Batch));
  mt_for_each_launch<Batch>(
      items, count, [](msclip_lamb_tensor& t, long long k) { t.p += k; t.n -= k; },
      [](const Batch& b, int nb, long long first_chunk) {
        for (int i = 0; i < nb; ++i) {
          const msclip_lamb_tensor& t = b.t[b.map[i] & 255u];
          printf("chunk %lld %lld %d %d\n", first_chunk + i, (long long)((unsigned long long)t.p >> 2) + (long long)(b.map[i] >> 8) * MT_CHUNK, t.param, t.adapt);
        }
      });
  return 0;
}
"""


def test_batcher_with_the_lamb_item(tmp_path):
    """Block b of a launch writes the partials of chunk first_chunk + b: across the cuts that 32 items / 400 chunks per launch
    make, that index is the chunk's position in table order, which is what first_chunk_dev ranges over.  The limits are read
    from optim.hip, so the size checked is the size launched."""
    with open(os.path.join(ROOT, "msclip_amd", "csrc", "optim.hip")) as f:
        NT, NB = map(int, re.search(r"using LambBatch = MtBatch<msclip_lamb_tensor, (\d+), (\d+)>;", f.read()).groups())
    assert NT < 36                                                         # 72-byte items: fewer fit than AdamW's
    (tmp_path / "batch.cpp").write_text(_BATCH_PROGRAM.replace("NT_", str(NT)).replace("NB_", str(NB)))
    cxx = shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, or the clang++ that hipcc drives)"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "msclip_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    str(tmp_path / "batch.cpp"), "-o", str(tmp_path / "batch")], check=True)
    C = 32768
    ns = [1, C, C + 1, (NB + 3) * C + 5] + [7] * (2 * NT + 1) + [2 * NB * C]     # cuts by the chunk limit and by the item limit
    out = subprocess.run([str(tmp_path / "batch")], input=" ".join(map(str, ns)), check=True, capture_output=True, text=True).stdout
    first, *rows = out.splitlines()
    assert first.startswith("sizeof ") and int(first.split()[1]) == 72 * NT + 4 * NB <= 4000
    got = [tuple(int(x) for x in r.split()[1:]) for r in rows]
    expect = [((i << 32) + c * C, i // 2, i & 1) for i, n in enumerate(ns) for c in range(-(-n // C))]
    assert [g[1:] for g in got] == expect
    assert [g[0] for g in got] == list(range(len(expect)))


# ---------------------------------------------------------------------------- checkpoint
def _stub(optimizer, clip=None):
    p = {"w": torch.nn.Parameter(torch.ones(3)), "b": torch.nn.Parameter(torch.zeros(2))}
    ts = types.SimpleNamespace(optimizer=optimizer, steps=4, bn="frozen", betas=(0.9, 0.98), eps=1e-6, trust_clip=True,
                               always_adapt=False, clip_grad_norm=clip, ema_shadow=None, _dp_gen=None,
                               state={"w": (torch.full((3,), 2.0), torch.full((3,), 3.0))},
                               param_groups=lambda: [("w", p["w"], 1e-3, 0.05), ("b", p["b"], 1e-3, 0.0)],
                               _ema_live=lambda what: None)
    return ts


def test_checkpoint_optimizer_block():
    adamw = train._optimizer_state_dict(_stub("adamw"))
    assert adamw["msclip"] == {"steps": 4, "bn": "frozen", "names": ["w", "b"]}                  # as before lamb existed
    assert adamw["param_groups"] == [
        {"lr": 1e-3, "weight_decay": 0.05, "betas": (0.9, 0.98), "eps": 1e-6, "amsgrad": False, "params": [0]},
        {"lr": 1e-3, "weight_decay": 0.0, "betas": (0.9, 0.98), "eps": 1e-6, "amsgrad": False, "params": [1]}]
    lamb = train._optimizer_state_dict(_stub("lamb", clip=2.0))
    assert lamb["msclip"] == {"steps": 4, "bn": "frozen", "names": ["w", "b"], "optimizer": "lamb"}
    keys = dict(bias_correction=True, betas=(0.9, 0.98), eps=1e-6, grad_averaging=True, max_grad_norm=2.0, trust_clip=True,
                always_adapt=False)
    assert lamb["param_groups"] == [dict(keys, lr=1e-3, weight_decay=0.05, params=[0]), dict(keys, lr=1e-3, weight_decay=0.0, params=[1])]
    assert train._optimizer_state_dict(_stub("lamb"))["param_groups"][0]["max_grad_norm"] is None
    assert set(lamb["state"]) == {0} and torch.equal(lamb["state"][0]["exp_avg_sq"], torch.full((3,), 3.0))


def test_resume_refuses_another_optimizers_checkpoint(tmp_path):
    for wrote, runs in (("lamb", "adamw"), ("adamw", "lamb")):
        path = str(tmp_path / f"{wrote}.pth")
        torch.save({"step": 5, "state_dict": {}, "optimizer": train._optimizer_state_dict(_stub(wrote))}, path)
        with pytest.raises(ValueError, match=wrote):
            train.resume_checkpoint(None, _stub(runs), path)
