"""TrainStep's gradients, EVERY element, against autograd of the oracle (real MI355X).

The sampled fixture tests (test_gpu_train.py, test_gpu_train_l14.py) compare against autograd of the real reference, of which
the fixtures keep 64 points per weight matrix: a zeroed head, q rows scaled by 15 % or a lost 4-row tile tail can pass them
(tests/test_gradcheck_cpu.py plants such defects and requires the bounds used here to report them).  Here the reference is
oracle/autograd.py -- the reference's autograd to fp32 rounding (tests/test_oracle_autograd_cpu.py) -- which gives every
element, at any batch and seed; it runs on the CPU, in fp32 for the reference and once more under bf16 autocast for the
yardstick.  Metrics and bounds: tests/gradcheck.py; cases: tests/train_full_cases.py.

r, the factor allowed on a tensor's own yardstick value, is measured, not chosen: tools/train_full_gradient_ratios.py runs
these cases and writes the distribution of engine / yardstick to tests/golden/train_full_gradient_ratios.json; r = 1.25 x the
measured worst, at most 2.  "Worst" is taken over the tensors whose own block error exceeds the bound's additive margin
(gradcheck.OWN_MARGIN = 0.02): below it `block error <= r x yardstick + 0.02` holds for any r, so the ratio says nothing.
That leaves out logit_scale at 7.4 x (ViT-B/32, batch 32, frozen) and 66 x (ViT-L/14) its yardstick, both listed in the JSON's
"scalar" class: one number, a sum of cancelling terms, 0.0169 and 0.0041 from the reference where the yardstick happened
to land 0.0023 and 0.00006 from it -- one draw of a signed error near zero, not a scale.  Every tensor, those included, is
asserted against r x its own yardstick + 0.02.

Cases: ViT-B/32 at batch 32 (the fixtures' seed) and at an odd batch (7: ragged GEMM tiles, padded weight-gradient contractions,
un-foldable BatchNorm maps), frozen and batch statistics; ViT-B/16 (197-token grid) frozen at 4 and batch statistics at 8; ViT-L/14
(257 tokens, patch convolution) at 4."""
import json

import pytest

import gradcheck as G
from train_full_cases import CASES, RATIOS, case_id, run_case

pytestmark = pytest.mark.gpu
# Tensors allowed more than the class-worst bound, by name, each with its reason: {case id: {parameter: extra block error}}.
# The bound r x the tensor's own yardstick value takes no exception: no tensor needed one.
EXCEPTIONS = {
    # ViT-B/16, frozen statistics, batch 4: bn1.bias of the parallel branch's second bottleneck is one number per channel, the sum
    # of a bf16 gradient map over 4 x 56 x 56 pixels whose terms nearly cancel.  It is the yardstick's own second-noisiest
    # conv-side tensor (0.1796; the noisiest, bn2.weight of the same block, 0.1816), TrainStep's is 0.2218 = 1.24 x its own
    # yardstick value, far inside r; only "no worse than the worst of the class + 0.04" trips, by 0.0002 -- at batch 4 that
    # maximum over 114 tensors is decided by one or two of them.  The allowance is 5e-3, the smallest margin these bounds use
    # anywhere (gradcheck.MEDIAN_MARGIN, COS_MARGIN); both sides are deterministic, so nothing larger is needed.
    "b16-frozen-b4": {"visual.transformer.parallel_branch_v.2.resnet_stage.conv_0.bn1.bias": 5e-3},
}


def load_r():
    with open(RATIOS) as f:
        d = json.load(f)
    assert 0 < d["r"] <= G.R_MAX and abs(d["r"] - min(G.R_MAX, 1.25 * d["measured_worst_ratio"])) < 1e-9
    return d["r"]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_every_gradient_element_against_oracle_autograd(gpu_device, case):
    got, yard, loss, ref_loss, secs = run_case(case)
    cid = case_id(case)
    print(f"{cid}: loss {loss:.5f} (oracle {ref_loss:.5f}); oracle passes + metrics on the CPU {secs:.1f} s")
    print(G.describe(cid, got, yard))
    assert abs(loss - ref_loss) <= 2e-2, (loss, ref_loss)
    bad = G.violations(got, yard, load_r(), EXCEPTIONS.get(cid))
    assert not bad, "\n".join(bad)
