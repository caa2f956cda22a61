"""Cross-check of the oracle against the reference on another weight seed and batch: the reference's features are stored in
tests/golden/b32-yfcc-msclips.xcheck_seed7.npz (tools/make_golden.py --oracle-xcheck), so the test needs no reference tree."""
import os

import numpy as np
import torch

from conftest import GOLDEN, load_schema
from msclip_amd import synth
from oracle import msclip_oracle as O


def test_b32_other_seed_and_batch():
    g = np.load(os.path.join(GOLDEN, "b32-yfcc-msclips.xcheck_seed7.npz"))
    sd = synth.synth_state_dict(load_schema("b32-yfcc-msclips"), seed=int(g["seed"]))
    img = synth.synth_images(2, seed=int(g["image_seed"]))
    tok = synth.synth_tokens(3, seed=int(g["token_seed"]))
    with torch.no_grad():
        oi, ot = O.encode_image(img, sd, O.arch_b32()), O.encode_text(tok, sd, O.arch_b32())
    ri, rt = torch.from_numpy(g["image_features"]), torch.from_numpy(g["text_features"])
    assert oi.shape == ri.shape and ot.shape == rt.shape
    assert (ri - oi).abs().max() < 1e-5
    assert (rt - ot).abs().max() < 1e-5
