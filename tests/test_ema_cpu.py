"""The weight EMA (TRAIN.EMA_DECAY) without a GPU: the extension header include/msclip_ext.h as msclip_amd/abi.py binds it, the
C layout of msclip_ema_tensor, the library's exports, msclip_ema_multi's argument validation (which runs on the host, before
any launch), TrainStep's / from_config's handling of the value, and the fp32 coefficients that EmaPlan passes."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from msclip_amd import abi, hip, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config

B32 = "b32-yfcc-msclips"
VP, CI, CF, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


def _lib():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    return hip.lib()


def test_extension_header_binding():
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    assert os.path.basename(abi.EXT_HEADER) == "msclip_ext.h" and os.path.dirname(abi.EXT_HEADER) == os.path.dirname(abi.HEADER)
    assert ext.version == 1
    assert list(ext.structs) == ["msclip_ema_tensor"]
    assert ext.structs["msclip_ema_tensor"]._fields_ == [("ema", VP), ("p", VP), ("n", LL)]
    assert ext.protos == {"msclip_ema_multi": (CI, [VP, CI, CF, CF, VP]), "msclip_ext_abi_version": (CI, [])}
    assert hip.EXT_EXPORTS == ("msclip_ema_multi", "msclip_ext_abi_version") and hip.EXT_ABI_VERSION == 1
    assert hip.EmaTensor is hip._EXT.structs["msclip_ema_tensor"]
    with pytest.raises(abi.AbiError):                                  # each header is read with its own version macro only
        abi.load(abi.EXT_HEADER)
    with pytest.raises(abi.AbiError):
        abi.load(abi.HEADER, abi.EXT_VERSION_MACRO)
    # the main table keeps describing msclip_hip.h alone
    main = abi.load()
    assert main.version == 9 == hip.ABI_VERSION and len(main.protos) == 107 == len(hip.EXPORTS) and len(main.structs) == 9
    assert not set(ext.protos) & set(main.protos) and "msclip_ema_tensor" not in hip._ABI.structs


def test_ema_tensor_matches_the_c_compilers_layout(tmp_path):
    """sizeof / offsetof as a host C compiler sees include/msclip_ext.h (plain C99) against the ctypes mirror: the method of
    tests/test_host_cpu.py::test_struct_mirrors_match_the_c_compilers_layout."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "msclip_ext.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(msclip_ema_tensor));']
    expect = [str(ctypes.sizeof(hip.EmaTensor))]
    for field, _ in hip.EmaTensor._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(msclip_ema_tensor, {field}));')
        expect.append(f"{field} {getattr(hip.EmaTensor, field).offset}")
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    cc = shutil.which("cc") or "/opt/rocm/lib/llvm/bin/clang"
    assert os.path.exists(cc), "no host C compiler (cc, or the clang that hipcc drives)"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"),
                    "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert got == expect == ["24", "ema 0", "p 8", "n 16"]


def test_library_exports_the_extension():
    L = _lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.EXT_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_ext_abi_version() == 1
    assert list(L.msclip_ema_multi.argtypes) == [VP, CI, CF, CF, VP] and L.msclip_ema_multi.restype is CI
    assert L.msclip_abi_version() == 9


def test_library_without_the_extension_is_refused(monkeypatch):
    _lib()
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "_EXT", hip._EXT._replace(protos={**hip._EXT.protos, "msclip_not_built": (CI, [])}))
    with pytest.raises(hip.HipUnavailable, match=r"msclip_not_built.*msclip_ext\.h.*rebuild"):
        hip.lib()
    monkeypatch.undo()
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "EXT_ABI_VERSION", 2)
    with pytest.raises(hip.HipUnavailable, match=r"extension ABI version 1.*needs 2.*rebuild"):
        hip.lib()


def test_ema_multi_rejects_bad_arguments_before_launching():
    """Every rejection of include/msclip_ext.h's msclip_ema_multi, on fake non-null pointers: nothing launches."""
    L = _lib()
    EINVAL = -1
    good, good2, odd = 0x10000, 0x20004, 0x10002

    def table(*items):
        arr = (hip.EmaTensor * len(items))()
        for a, (e, p, n) in zip(arr, items):
            a.ema, a.p, a.n = e, p, n
        return arr

    def call(arr, count, d=0.5, omd=0.5):
        return L.msclip_ema_multi(arr, count, d, omd, None)
    ok = (good, good2, 8)
    assert call(None, 1) == EINVAL                                     # null table with count > 0
    assert call(table(ok), -1) == EINVAL                               # count < 0
    assert call(table(ok, (None, good2, 8)), 2) == EINVAL              # a null pointer in an item, either side
    assert call(table((good, None, 8), ok), 2) == EINVAL
    assert call(table(ok, (good, good2, 0)), 2) == EINVAL              # n <= 0
    assert call(table((good, good2, -5)), 1) == EINVAL
    assert call(table((odd, good2, 8)), 1) == EINVAL                   # not 4-byte aligned, either side
    assert call(table(ok, (good, odd, 8)), 2) == EINVAL
    nan = float("nan")
    for d in (-0.25, 1.5, nan, float("inf")):                          # decay / one_minus_decay outside [0, 1], or NaN
        assert call(table(ok), 1, d=d) == EINVAL, d
        assert call(table(ok), 1, omd=d) == EINVAL, d


def test_train_step_validates_ema_decay_before_any_gpu_use():
    model = get_clip_model(named_config(B32))                          # on the CPU: TrainStep would fail at model.engine()
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            train.TrainStep(model, lr=1e-4, ema_decay=bad)
    assert model._engine is None
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            hip.EmaPlan.coefficients(bad)


def test_config_reads_ema_decay():
    assert train.ema_setting(named_config(B32)) is None                                   # no key: off
    assert train.ema_setting(named_config(B32, ["TRAIN.EMA_DECAY", "0.0"])) is None       # the reference's default: off
    assert train.ema_setting(named_config(B32, ["TRAIN.EMA_DECAY", "0.9999"])) == 0.9999


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999, 0.99999])
def test_one_minus_decay_is_rounded_once_from_double(decay, monkeypatch):
    """What EmaPlan.run hands to msclip_ema_multi, seen through a stand-in library: decay as fp32, and float32(1.0 - decay) with
    the difference taken in double -- not 1 - float32(decay), which is another fp32 number for every value here but 0.5."""
    seen = []

    class Lib:
        @staticmethod
        def msclip_ema_multi(arr, n, d, omd, stream):
            seen.append((n, ctypes.c_float(d).value, ctypes.c_float(omd).value))
            return 0
    plan = hip.EmaPlan([], [])
    plan.n, plan.device = 1, None                                      # an empty table that is run as if it held a tensor
    monkeypatch.setattr(hip, "lib", lambda: Lib)
    monkeypatch.setattr(hip, "_stream", lambda: None)
    monkeypatch.setattr(hip.torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    plan.run(decay)
    assert seen == [(1, float(np.float32(decay)), float(np.float32(1.0 - decay)))]
    assert hip.EmaPlan.coefficients(decay) == seen[0][1:]
