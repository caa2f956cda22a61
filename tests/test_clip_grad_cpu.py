"""Gradient clipping by the global norm, the part that needs no GPU: include/msclip_hip_optim.h as the third ABI table
(its own version macro, its own exports, the first two tables untouched), the struct layout against a host C compiler,
the built library's symbols and host-side argument validation, and TRAIN.CLIP_GRAD_NORM in the config."""
import ctypes
import keyword
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from msclip_amd import abi, hip
from msclip_amd.config import default_config, named_config


def _optim_header_text():
    with open(abi.OPTIM_HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_third_header_parses_under_its_own_macro_and_leaves_the_other_tables_alone():
    t = abi.load(abi.OPTIM_HEADER, abi.OPTIM_VERSION_MACRO)
    assert os.path.basename(abi.OPTIM_HEADER) == "msclip_hip_optim.h" and abi.OPTIM_VERSION_MACRO == "MSCLIP_OPTIM_ABI_VERSION"
    assert t.version == hip.OPTIM_ABI_VERSION == hip._OPTIM_ABI.version == 1
    declared = set(re.findall(r"\b(msclip_[a-z0-9_]+)\s*\(", _optim_header_text()))
    assert declared == set(t.protos) == set(hip.OPTIM_EXPORTS) and tuple(t.protos) == hip.OPTIM_EXPORTS
    assert declared == {"msclip_grad_sumsq", "msclip_clip_coef", "msclip_adamw_multi_clipped", "msclip_optim_abi_version"}
    assert not declared & set(hip.EXPORTS) and not declared & set(hip.TRAIN_EXPORTS)
    vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    assert t.protos["msclip_grad_sumsq"] == (ci, [vp, ci, vp, ll, vp])
    assert t.protos["msclip_clip_coef"] == (ci, [vp, ll, cf, vp, vp])
    assert t.protos["msclip_adamw_multi_clipped"] == (ci, [vp, ci, cf, cf, cf, ci, vp, vp])
    assert t.protos["msclip_optim_abi_version"] == (ci, [])
    # the first two tables: unchanged
    first, second = abi.load(), abi.load(abi.TRAIN_HEADER, abi.TRAIN_VERSION_MACRO)
    assert len(hip.EXPORTS) == len(first.protos) == 103 and hip.ABI_VERSION == first.version == 8
    assert len(hip.TRAIN_EXPORTS) == len(second.protos) == 2 and hip.TRAIN_ABI_VERSION == second.version == 1
    assert len(first.structs) == 7 and set(second.structs) == {"msclip_accum_tensor"}
    assert not set(t.structs) & (set(first.structs) | set(second.structs))
    # each header under its own macro only
    for path, macro in ((abi.OPTIM_HEADER, abi.VERSION_MACRO), (abi.OPTIM_HEADER, abi.TRAIN_VERSION_MACRO),
                        (abi.HEADER, abi.OPTIM_VERSION_MACRO), (abi.TRAIN_HEADER, abi.OPTIM_VERSION_MACRO)):
        with pytest.raises(abi.AbiError):
            abi.load(path, macro)


def test_third_headers_structs_match_the_c_compilers_layout(tmp_path):
    bodies = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}", _optim_header_text()))
    structs = abi.load(abi.OPTIM_HEADER, abi.OPTIM_VERSION_MACRO).structs
    assert set(bodies) == set(structs) == {"msclip_sumsq_tensor"} and hip.SumsqTensor is hip._OPTIM_ABI.structs["msclip_sumsq_tensor"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "msclip_hip_optim.h"', "int main(void) {"]
    expect = []
    for cname, mirror in structs.items():
        assert len(mirror._fields_) == bodies[cname].count(";") + bodies[cname].count(",")
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        expect.append(f"{cname} {ctypes.sizeof(mirror)}")
        for field, _ in mirror._fields_:
            member = field[:-1] if keyword.iskeyword(field[:-1]) else field
            lines.append(f'  printf("{cname}.{member} %zu\\n", offsetof({cname}, {member}));')
            expect.append(f"{cname}.{member} {getattr(mirror, field).offset}")
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    cc = shutil.which("cc") or "/opt/rocm/lib/llvm/bin/clang"
    assert os.path.exists(cc), "no host C compiler (cc, or the clang that hipcc drives)"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"),
                    "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert got == expect and "msclip_sumsq_tensor 16" in got


def test_library_exports_the_third_headers_symbols_and_validates_on_the_host(monkeypatch):
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.OPTIM_EXPORTS:
        assert hasattr(lib, name), name
    lib.msclip_optim_abi_version.restype = ctypes.c_int
    assert lib.msclip_optim_abi_version() == hip.OPTIM_ABI_VERSION
    L = hip.lib()                                            # bound with the same rule as the other two tables
    for n, (r, a) in hip._OPTIM_ABI.protos.items():
        assert list(getattr(L, n).argtypes) == a and getattr(L, n).restype is r
    # host-side argument validation: -1 before any launch (no device is touched: these run without a GPU)
    one = (hip.SumsqTensor * 1)()
    one[0].g, one[0].n = 4096, 16
    assert L.msclip_grad_sumsq(None, 1, 8192, 1, None) == -1              # null table
    assert L.msclip_grad_sumsq(one, -1, 8192, 1, None) == -1              # count < 0
    assert L.msclip_grad_sumsq(one, 1, None, 1, None) == -1               # null partials
    assert L.msclip_grad_sumsq(one, 1, 8192, 2, None) == -1               # n_partials is not the chunk count
    one[0].g = 4097                                                       # not 4-byte aligned
    assert L.msclip_grad_sumsq(one, 1, 8192, 1, None) == -1
    one[0].g, one[0].n = 4096, 0
    assert L.msclip_grad_sumsq(one, 1, 8192, 0, None) == -1               # an empty tensor
    assert L.msclip_clip_coef(None, 1, 1.0, 8192, None) == -1 and L.msclip_clip_coef(4096, 1, 1.0, None, None) == -1
    assert L.msclip_clip_coef(4096, 0, 1.0, 8192, None) == -1 and L.msclip_clip_coef(4096, 1, -1.0, 8192, None) == -1
    assert L.msclip_clip_coef(4096, 1, float("nan"), 8192, None) == -1
    aw = (hip.AdamwTensor * 1)()
    aw[0].p, aw[0].g, aw[0].m, aw[0].v, aw[0].n = 4096, 8192, 12288, 16384, 16
    assert L.msclip_adamw_multi_clipped(None, 1, 0.9, 0.999, 1e-8, 1, 4096, None) == -1     # null table
    assert L.msclip_adamw_multi_clipped(aw, -1, 0.9, 0.999, 1e-8, 1, 4096, None) == -1      # count < 0
    assert L.msclip_adamw_multi_clipped(aw, 1, 0.9, 0.999, 1e-8, 1, None, None) == -1       # null coef
    assert L.msclip_adamw_multi_clipped(aw, 1, 0.9, 0.999, 1e-8, 0, 4096, None) == -1       # step < 1
    aw[0].g = 0
    assert L.msclip_adamw_multi_clipped(aw, 1, 0.9, 0.999, 1e-8, 1, 4096, None) == -1       # null gradient
    # a declared symbol that the library lacks gets the rebuild hint, naming the third header
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "_OPTIM_ABI", hip._OPTIM_ABI._replace(protos={**hip._OPTIM_ABI.protos, "msclip_not_built": (ctypes.c_int, [])}))
    with pytest.raises(hip.HipUnavailable, match="msclip_not_built.*msclip_hip_optim.h.*rebuild"):
        hip.lib()


def test_clip_grad_norm_in_the_config():
    from msclip_amd import train
    assert default_config().TRAIN.CLIP_GRAD_NORM == 0.0
    off, on = named_config("b32-yfcc-msclips"), named_config("b32-yfcc-msclips", ["TRAIN.CLIP_GRAD_NORM", "1.0"])
    assert off.TRAIN.CLIP_GRAD_NORM == 0.0 and on.TRAIN.CLIP_GRAD_NORM == 1.0
    seven = dict(lr=0.0001, lr_share=0.0001, wd=0.05, wd_share=0.2, betas=(0.9, 0.999), eps=1e-8, without_wd=("bn", "bias", "ln"))
    assert train.optimizer_settings(off) == seven and train.optimizer_settings(on) == seven


def test_train_step_takes_clip_grad_norm_and_refuses_a_negative_one():
    import inspect
    from msclip_amd import train
    sig = inspect.signature(train.TrainStep.__init__)
    assert sig.parameters["clip_grad_norm"].default is None
    assert inspect.signature(hip.AdamwPlan.run).parameters["max_norm"].default is None
    with pytest.raises(ValueError, match="clip_grad_norm"):
        train.TrainStep(None, clip_grad_norm=-1.0)
