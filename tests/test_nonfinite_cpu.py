"""The non-finite guard of the optimizer phase (TrainStep(nonfinite=...)) without a GPU: the fourth extension header's binding,
the library's exports and argument validation (which runs on the host, before any launch), the config reader, the chunk -> name
map, the checkpoint's optimizer block, and the torch restatement of the verdict that tests/test_gpu_nonfinite.py compares
the kernel with."""
import ctypes
import os
import types

import pytest
import torch

import nonfinite_ref as R
from msclip_amd import abi, hip, train
from msclip_amd.config import named_config

B32 = "b32-yfcc-msclips"
VP, CI, CF, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
CHUNK = 32768


# ---------------------------------------------------------------------------- the extension header
def test_guard_header_binding():
    main = abi.load()
    ext = abi.load(abi.EXT_HEADER, abi.EXT_VERSION_MACRO)
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    ext3 = abi.load(abi.EXT3_HEADER, abi.EXT3_VERSION_MACRO, known=tuple(main.structs))
    ext4 = abi.load(abi.EXT4_HEADER, abi.EXT4_VERSION_MACRO, known=tuple(main.structs) + tuple(ext3.structs))
    assert os.path.basename(abi.EXT4_HEADER) == "msclip_ext4.h" and ext4.version == 1 == hip.EXT4_ABI_VERSION
    assert not ext4.structs                                              # it declares no struct of its own
    assert ext4.protos == {
        "msclip_clip_coef_guarded": (CI, [VP, LL, CF, VP, VP, VP]),
        "msclip_adamw_multi_guarded": (CI, [VP, CI, CF, CF, CF, CI, VP, VP, VP]),
        "msclip_lamb_apply_guarded": (CI, [VP, CI, CF, CF, CF, CI, VP, VP, VP, VP]),
        "msclip_ext4_abi_version": (CI, []),
    }
    assert hip.EXT4_EXPORTS == tuple(ext4.protos)
    others = set(main.protos) | set(ext.protos) | set(ext2.protos) | set(ext3.protos)
    assert not set(ext4.protos) & others
    assert (set(hip.EXPORTS) | set(hip.EXT_EXPORTS) | set(hip.EXT2_EXPORTS) | set(hip.EXT3_EXPORTS)) == others
    # the older headers are what they were
    assert main.version == 9 and len(main.protos) == 107 and ext.version == 1 and ext2.version == 1 and ext3.version == 1
    assert len(ext.protos) == 2 and len(ext2.protos) == 4 and len(ext3.protos) == 4
    assert ctypes.sizeof(hip.AdamwTensor) == 64 and ctypes.sizeof(hip.LambTensor) == 72


def _tables():
    adam = (hip.AdamwTensor * 2)()
    lamb = (hip.LambTensor * 2)()
    for arr in (adam, lamb):
        for a, n in zip(arr, (5, 40000)):
            a.p = a.g = a.m = a.v = 0x10000
            a.n, a.lr = n, 1e-3
    lamb[0].param, lamb[1].param = 0, 1
    return adam, lamb


def test_library_exports_and_rejections():
    """Every MSCLIP_EINVAL rule on fake non-null pointers: a call that got past its checks would launch on them."""
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.EXT4_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_ext4_abi_version() == 1
    p, odd = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10002)
    # the verdict: msclip_clip_coef's rules, plus state non-null and 4-byte aligned
    for args in ((None, 1, 1.0, p, p), (p, 1, 1.0, None, p), (p, 1, 1.0, p, None), (p, 0, 1.0, p, p), (p, -3, 1.0, p, p),
                 (p, 1, -1.0, p, p), (p, 1, float("nan"), p, p), (odd, 1, 1.0, p, p), (p, 1, 1.0, odd, p), (p, 1, 1.0, p, odd)):
        assert L.msclip_clip_coef_guarded(*args, None) == -1, args
    adam, lamb = _tables()
    hyper = (0.9, 0.999, 1e-6)
    # guarded AdamW: the table's rules, step >= 1, skip_dev non-null and aligned, coef_dev NULL or aligned
    assert L.msclip_adamw_multi_guarded(None, 2, *hyper, 1, None, p, None) == -1
    assert L.msclip_adamw_multi_guarded(adam, -1, *hyper, 1, None, p, None) == -1
    assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 0, None, p, None) == -1
    assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 1, None, None, None) == -1
    assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 1, None, odd, None) == -1
    assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 1, odd, p, None) == -1
    for field, bad in (("p", None), ("g", None), ("m", None), ("v", None), ("n", 0)):
        adam, _ = _tables()
        setattr(adam[1], field, bad)
        assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 1, None, p, None) == -1, field
    adam, _ = _tables()
    adam[0].pk, adam[0].pk_f32 = 0x10000, 2
    assert L.msclip_adamw_multi_guarded(adam, 2, *hyper, 1, p, p, None) == -1
    # guarded LAMB apply: msclip_lamb_apply's rules, plus skip_dev
    assert L.msclip_lamb_apply_guarded(None, 2, *hyper, 1, None, p, p, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 0, None, p, p, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, None, p, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, odd, p, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, p, None, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, p, odd, None) == -1
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, odd, p, p, None) == -1
    lamb[1].param = 2                                                    # parameters are numbered without gaps
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, p, p, None) == -1
    lamb[1].param, lamb[0].g = 1, None
    assert L.msclip_lamb_apply_guarded(lamb, 2, *hyper, 1, None, p, p, None) == -1


# ---------------------------------------------------------------------------- config
def test_nonfinite_setting_from_the_config():
    assert train.nonfinite_setting(named_config(B32)) is None
    assert train.nonfinite_setting(named_config(B32, ["TRAIN.DETECT_ANOMALY", "False", "TRAIN.SKIP_NONFINITE", "False"])) is None
    assert train.nonfinite_setting(named_config(B32, ["TRAIN.SKIP_NONFINITE", "True"])) == "skip"
    assert train.nonfinite_setting(named_config(B32, ["TRAIN.DETECT_ANOMALY", "True"])) == "raise"
    assert train.nonfinite_setting(named_config(B32, ["TRAIN.DETECT_ANOMALY", "True", "TRAIN.SKIP_NONFINITE", "True"])) == "raise"
    assert train.NONFINITE == (None, "skip", "raise")


# ---------------------------------------------------------------------------- chunk -> name
def test_nonfinite_names_on_hand_made_partials():
    # first: one chunk; mid: three chunks; in_proj: the joined pieces, ONE entry of 2 chunks; tiny: one; last: two
    table = [("first", 5), ("mid", 2 * CHUNK + 1), ("in_proj", CHUNK + 10), ("tiny", 1), ("last", CHUNK + 1)]
    n = 1 + 3 + 2 + 1 + 2

    def names(*bad, value=float("nan")):
        part = torch.rand(n)
        for i in bad:
            part[i] = value
        return train.nonfinite_names(part, table)
    assert names() == []
    assert names(0) == ["first"]                                         # the first tensor
    assert names(8) == ["last"] and names(7, value=float("inf")) == ["last"]      # the last tensor, either chunk
    assert names(1) == ["mid"] and names(2) == ["mid"] and names(3, value=float("-inf")) == ["mid"]      # a multi-chunk tensor
    assert names(4) == ["in_proj"] and names(5) == ["in_proj"]          # the joined one: either piece names the parameter once
    assert names(4, 5) == ["in_proj"]
    assert names(6) == ["tiny"]
    assert names(8, 0, 5) == ["first", "in_proj", "last"]               # table order
    with pytest.raises(ValueError):
        train.nonfinite_names(torch.rand(n + 1), table)
    # the same map as the verdict's index
    part = torch.rand(n)
    part[5] = float("inf")
    part[7] = float("nan")
    assert R.verdict(part, 3) == [1, 4, 5, 2] and train.nonfinite_names(part, table) == ["in_proj", "last"]


def test_reference_verdict():
    part = torch.rand(300)
    assert R.verdict(part, 7) == [0, 7, -1, 0] and R.norm64(part) == pytest.approx(float(part.double().sum().sqrt()))
    for bad in (float("nan"), float("inf"), float("-inf")):
        q = part.clone()
        q[256] = bad
        assert R.verdict(q) == [1, 1, 256, 1] and not torch.isfinite(torch.tensor(R.norm64(q)))
    q = part.clone()
    q[299], q[17] = float("nan"), float("-inf")
    assert R.verdict(q, 2) == [1, 3, 17, 2]
    # the bit test is torch's isfinite, denormals and the largest finite value included
    edge = torch.tensor([0.0, -0.0, 1e-45, 3.4028234e38, -3.4028234e38, float("inf"), float("nan")])
    assert torch.equal(R.nonfinite_mask(edge), ~torch.isfinite(edge))


# ---------------------------------------------------------------------------- checkpoint
def _stub(nonfinite, optimizer="adamw", skipped=0):
    p = {"w": torch.nn.Parameter(torch.ones(3)), "b": torch.nn.Parameter(torch.zeros(2))}
    ts = types.SimpleNamespace(optimizer=optimizer, steps=6, bn="frozen", betas=(0.9, 0.98), eps=1e-6, trust_clip=False,
                               always_adapt=False, clip_grad_norm=None, ema_shadow=None, _dp_gen=None,
                               state={"w": (torch.full((3,), 2.0), torch.full((3,), 3.0))},
                               param_groups=lambda: [("w", p["w"], 1e-3, 0.05), ("b", p["b"], 1e-3, 0.0)],
                               _ema_live=lambda what: None)
    if nonfinite != "absent":
        ts.nonfinite, ts.skipped_steps = nonfinite, skipped
    return ts


def test_checkpoint_optimizer_block_with_and_without_the_guard():
    for kind, base in (("adamw", {"steps", "bn", "names"}), ("lamb", {"steps", "bn", "names", "optimizer"})):
        for off in (_stub(None, kind), _stub("absent", kind)):           # guard off: no trace of the feature
            d = train._optimizer_state_dict(off)
            assert set(d["msclip"]) == base and d["msclip"]["steps"] == 6 and float(d["state"][0]["step"]) == 6.0
        for mode in ("skip", "raise"):
            d = train._optimizer_state_dict(_stub(mode, kind, skipped=2))
            assert set(d["msclip"]) == base | {"skipped_steps"}
            assert d["msclip"]["steps"] == 6 and d["msclip"]["skipped_steps"] == 2
            assert float(d["state"][0]["step"]) == 4.0                   # the applied count
            assert set(d["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        assert train._optimizer_state_dict(_stub("skip", kind))["msclip"]["skipped_steps"] == 0
    assert set(train._optimizer_state_dict(_stub(None))["param_groups"][0]) == {"lr", "weight_decay", "betas", "eps", "amsgrad", "params"}
    assert train._optimizer_state_dict(_stub("skip"))["param_groups"] == train._optimizer_state_dict(_stub(None))["param_groups"]
