"""Gradient clipping by the global norm, the part that needs no GPU: host-side argument validation of the three entry
points (their signatures and struct layouts are pinned in tests/test_host_cpu.py) and TRAIN.CLIP_GRAD_NORM in the config."""
import os

import pytest

from msclip_amd import hip
from msclip_amd.config import default_config, named_config


def test_clipping_entry_points_validate_on_the_host():
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    L = hip.lib()
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
