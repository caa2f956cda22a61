"""Stochastic depth (MODEL.SPEC.VISION.DROP_PATH) without a GPU: the model factory, the config reader, the row-scale tables, the
row-scale extension header's binding, and the oracle helper (tests/droppath_ref.py) pinned against the real reference module."""
import ctypes
import os
import sys

import pytest
import torch

import droppath_ref as R
from conftest import ROOT, load_schema, synth_sd
from msclip_amd import abi, hip, synth, train
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config
from oracle import msclip_oracle as O

B32 = "b32-yfcc-msclips"
VP, CI, CF = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


# ---------------------------------------------------------------------------- factory, settings
def test_factory_accepts_drop_path_and_keeps_the_state_dict():
    m0 = get_clip_model(named_config(B32))
    m1 = get_clip_model(named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", "0.1"]))
    assert m0.drop_path == 0.0 and m1.drop_path == 0.1
    assert list(m0.state_dict()) == list(m1.state_dict())                  # timm's DropPath has no parameters or buffers
    assert [k for k, _ in m0.named_parameters()] == [k for k, _ in m1.named_parameters()]
    m1.load_state_dict(synth_sd(B32), strict=True)
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(ValueError, match="DROP_PATH"):
            get_clip_model(named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", bad]))


def test_drop_path_setting_reads_the_config():
    assert train.drop_path_setting(named_config(B32)) == 0.0
    assert train.drop_path_setting(named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", "0.2"])) == 0.2
    assert train.drop_path_setting(named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", "0"])) == 0.0
    with pytest.raises(ValueError):
        train.drop_path_setting(named_config(B32, ["MODEL.SPEC.VISION.DROP_PATH", "1.0"]))
    assert train.DROP_PATH_MODES == ("sample", "position")


# ---------------------------------------------------------------------------- tables
@pytest.mark.parametrize("mode", ["sample", "position"])
@pytest.mark.parametrize("keep", [0.75, 0.9, 1.0])
def test_drop_path_table(mode, keep):
    Bi, Lv, nb, Mt = 3, 5, 4, 11
    M = Bi * Lv + Mt
    n = Bi if mode == "sample" else Lv
    g = torch.Generator().manual_seed(1)
    draws = torch.rand(nb, 2, n, generator=g) < 0.5
    draws[0, 0] = True
    draws[1, 1] = False
    t = train.drop_path_table(draws, Bi, Lv, M, mode, keep)
    assert t.shape == (nb, 2, M) and t.dtype == torch.float32 and t.is_contiguous()
    assert bool((t[:, :, Bi * Lv:] == 1.0).all())                          # text rows, up to the launch's bound
    inv = torch.tensor(1.0 / keep, dtype=torch.float32)
    img = t[:, :, :Bi * Lv].view(nb, 2, Bi, Lv)
    assert bool(((img == 0) | (img == inv)).all())                         # exactly 0 or 1 / keep
    for b in range(Bi):
        for l in range(Lv):
            d = draws[:, :, b] if mode == "sample" else draws[:, :, l]
            assert torch.equal(img[:, :, b, l] != 0, d)
    # the compact last block: the table gathered with the live-row list equals the full table at those rows
    crow = torch.cat([torch.arange(0, Bi * Lv, Lv), torch.tensor([Bi * Lv + 2, Bi * Lv + 4, Bi * Lv + 10])])
    compact = torch.stack([t[nb - 1, 0], t[nb - 1, 1]]).index_select(1, crow)
    for k in range(2):
        for j, r in enumerate(crow.tolist()):
            assert compact[k, j] == t[nb - 1, k, r]
    assert bool((compact[:, Bi:] == 1.0).all())


def test_drop_path_table_rejects_bad_input():
    ok = torch.ones(2, 2, 3, dtype=torch.bool)
    with pytest.raises(ValueError):
        train.drop_path_table(ok, 3, 5, 15, "token", 0.9)
    with pytest.raises(ValueError):
        train.drop_path_table(ok, 4, 5, 20, "sample", 0.9)                 # 3 draws for 4 images
    with pytest.raises(ValueError):
        train.drop_path_table(ok.float(), 3, 5, 15, "sample", 0.9)
    with pytest.raises(ValueError):
        train.drop_path_table(ok, 3, 5, 14, "sample", 0.9)                 # M below the image rows
    with pytest.raises(ValueError):
        train.drop_path_table(ok, 3, 5, 15, "sample", 0.0)


# ---------------------------------------------------------------------------- the extension header's binding
def test_rowscale_header_binding():
    main = abi.load()
    ext2 = abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO, known=tuple(main.structs))
    assert os.path.basename(abi.EXT2_HEADER) == "msclip_ext2.h" and ext2.version == 1 == hip.EXT2_ABI_VERSION
    assert ext2.structs == {}
    ln_bwd = main.protos["msclip_layernorm_bwd"][1]
    cast = main.protos["msclip_cast_bf16_colsum"][1]
    assert ext2.protos == {
        "msclip_gemm_rowscale": (CI, [VP, VP, VP]),
        "msclip_layernorm_bwd_rowscale": (CI, ln_bwd[:-1] + [VP, VP]),     # the parent entry point's arguments, then the scale
        "msclip_cast_bf16_colsum_rowscale": (CI, cast[:-1] + [VP, VP]),
        "msclip_ext2_abi_version": (CI, []),
    }
    assert hip.EXT2_EXPORTS == tuple(ext2.protos)
    assert not set(ext2.protos) & (set(main.protos) | set(hip.EXT_EXPORTS))
    with pytest.raises(abi.AbiError):                                      # its prototypes point to msclip_gemm_desc: unknown on its own
        abi.load(abi.EXT2_HEADER, abi.EXT2_VERSION_MACRO)
    # the headers that earlier tests pin are what they were
    assert main.version == 9 and len(main.protos) == 107 and ctypes.sizeof(hip.GemmDesc) == 280


def test_library_exports_the_rowscale_entry_points():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in hip.EXT2_EXPORTS:
        assert hasattr(raw, name), name
    assert L.msclip_ext2_abi_version() == 1
    # rejected before anything launches (fake non-null pointers): a scale on the LayerNorm backward without the bf16 copy
    p = ctypes.c_void_p(0x10000)
    rc = L.msclip_layernorm_bwd_rowscale(p, 768, None, 1, p, 768, 1, p, p, 768, 1, None, 1024, 8, 768, 1e-12, None, 0, None, 0, p, None)
    assert rc == -1


# ---------------------------------------------------------------------------- the helper against the real reference
def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ref_import
    finally:
        sys.path.pop(0)
    return ref_import


def test_mixed_masks_drop_and_keep_in_every_block():
    for mode, batch in (("sample", 4), ("sample", 2), ("position", 4)):
        m = R.mixed_masks(O.arch_b32(), batch, mode)
        assert tuple(m.shape) == R.mask_shape(O.arch_b32(), batch, mode) and m.shape[0] == 11
        assert bool(m.any(-1).all()) and bool((~m).any(-1).all())
    assert R.mask_shape(O.arch_l14(), 2, "sample") == (24, 2, 2) and R.mask_shape(O.arch_l14(), 2, "position") == (24, 2, 257)


def test_helper_position_mode_is_the_reference_module_with_drop_path():
    """The reference B/32 model built with DROP_PATH = 0.25, its transformer blocks in train(), timm's DropPath replaced by a stub
    that multiplies by a replayed mask of shape (x.shape[0], 1, 1) / keep: the module's blocks run sequence-first, so dimension 0
    is the token position.  The helper in "position" mode must give the same image features (the bound this suite uses for the
    oracle against the reference: 1e-5)."""
    ref_import = _reference()
    if not ref_import.reference_available():
        pytest.skip("reference tree absent")
    M = ref_import.import_reference_module()
    p, keep = 0.25, 0.75
    arch = O.arch_b32()
    masks = R.mixed_masks(arch, 3, "position", seed=4)
    queue, seen = [], []

    class ReplayDropPath(torch.nn.Module):
        def __init__(self, drop_prob=0.0):
            super().__init__()
            self.drop_prob = drop_prob

        def forward(self, x):
            if not self.training:
                return x
            r = queue.pop(0)
            seen.append(tuple(x.shape))
            assert r.numel() == x.shape[0]
            return x * (r.to(x.dtype).view(x.shape[0], 1, 1) / (1.0 - self.drop_prob))

    cfg = ref_import.load_reference_config(B32)
    cfg["MODEL"]["SPEC"]["VISION"]["DROP_PATH"] = p
    old = M.DropPath
    M.DropPath = ReplayDropPath
    try:
        model = M.get_clip_model(cfg).eval()
    finally:
        M.DropPath = old
    sd = synth.synth_state_dict(load_schema(B32), seed=0)
    model.load_state_dict(sd, strict=True)
    blocks = list(model.visual.transformer.resblocks)[1:]
    assert all(isinstance(b.drop_path, ReplayDropPath) for b in blocks)
    assert not any(isinstance(b.drop_path, ReplayDropPath) for b in model.transformer.resblocks)       # the text tower has none
    for b in blocks:
        b.train()
    img = synth.synth_images(3, seed=11)
    queue.extend(masks[vi, k] for vi in range(masks.shape[0]) for k in range(2))
    with torch.no_grad():
        want = model.encode_image(img)
    assert not queue and all(s[0] == 50 and s[1] == 3 for s in seen)       # dimension 0 of the reference's blocks: 50 token positions
    tok = synth.synth_tokens(3, seed=12)
    got, _, _ = R.droppath_forward(sd, arch, img, tok, masks, "position", keep)
    plain = O.encode_image(img, sd, arch)
    print("helper vs reference with DropPath:", float((got - want).abs().max()), "; drop path moved the features by",
          float((plain - want).abs().max()))
    assert float((got - want).abs().max()) <= 1e-5
    assert float((plain - want).abs().max()) > 1e-3                        # the masks did act


# ---------------------------------------------------------------------------- the gradient check has teeth
def test_bias_sums_without_the_scale_fall_outside_the_gradient_bounds():
    """tests/test_gpu_droppath.py holds TrainStep's gradients to tests/gradcheck.py's bounds against the helper's autograd.  In the
    style of tests/test_gradcheck_cpu.py: the stand-in for a correct bf16 implementation (the helper under bf16 autocast) passes
    every bound; the same run with the row scale left out of the bias sums of out_proj / c_proj -- forward unchanged -- is
    reported, for those bias tensors of the vision-only and shared blocks and for nothing else."""
    import gradcheck as G
    from oracle.autograd import parameter_aliases
    arch = O.arch_b32()
    m = get_clip_model(named_config(B32))
    alias = parameter_aliases(m)
    img, tok = synth.synth_images(8, seed=0), synth.synth_tokens(8, seed=1)
    masks = R.mixed_masks(arch, 8, "sample", seed=2)
    args = (synth_sd(B32), arch, img, tok, masks, "sample", 0.75)
    ref, _ = R.droppath_gradients(*args, aliases=alias)
    yard, _ = R.droppath_gradients(*args, aliases=alias, autocast_bf16=True)
    broken, _ = R.droppath_gradients(*args, aliases=alias, autocast_bf16=True, bias_unscaled=True)
    ym = G.measure(yard, ref)
    assert G.violations(ym, ym, G.R_MAX) == []
    bad = G.violations(G.measure(broken, ref), ym, G.R_MAX)
    keys = sorted({line.split(":")[0] for line in bad})
    print(len(bad), "violations in", len(keys), "tensors, e.g.", bad[:3])
    biases = [f"visual.transformer.resblocks.{i}.{leaf}" for i in range(1, 12) for leaf in ("attn.out_proj.bias", "mlp.c_proj.bias")]
    assert keys and set(keys) <= set(biases), [k for k in keys if k not in biases]
    assert len(keys) >= 11                                                 # at least every second one of the 22 (mixed masks: each drops and keeps)
