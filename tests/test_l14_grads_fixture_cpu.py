"""The L/14 gradient fixture (tests/golden/l14-fp8-msclips.grads.npz, tools/make_golden.py --grads-l14) covers exactly the
parameters of the model this build makes from experiments/model/l14-fp8-msclips.yaml (no GPU needed)."""
import os

import numpy as np

from conftest import GOLDEN
from msclip_amd.clip_openai_pe_res_v1 import get_clip_model
from msclip_amd.config import named_config


def test_l14_grads_fixture_covers_every_parameter():
    g = np.load(os.path.join(GOLDEN, "l14-fp8-msclips.grads.npz"))
    keys = {k[2:] for k in g.files if k.startswith("g_")}
    m = get_clip_model(named_config("l14-fp8-msclips", ["MODEL.SPEC.PRECISION", "bf16"]))
    params = dict(m.named_parameters())                       # aliases resolved: one name per Parameter object
    assert len(keys) == 406 and keys == set(params)
    assert "visual.conv1.weight" in keys and tuple(params["visual.conv1.weight"].shape) == (1024, 3, 14, 14)
    # the text-tower names of the shared tensors point at their visual.* entry
    aliases = {k[6:]: str(g[k]) for k in g.files if k.startswith("alias_")}
    all_names = dict(m.named_parameters(remove_duplicate=False))
    assert aliases and all(a in all_names and v in keys and all_names[a] is all_names[v] for a, v in aliases.items())
    assert int(g["batch"]) == 4 and np.isfinite(float(g["loss"]))
    assert os.path.getsize(os.path.join(GOLDEN, "l14-fp8-msclips.grads.npz")) < 1 << 20
