"""Measure TrainStep.accumulate's gradients against the yardstick on an MI355X:

    python tools/accumulate_gradient_ratios.py [out.json]        # default: tests/golden/accumulate_gradient_ratios.json

Runs the cases of tests/test_gpu_accumulate.py (tests/accumulate_cases.py) once and writes, per case and tensor class, the
distribution of `block error of accumulate() / block error of the yardstick` as tools/train_full_gradient_ratios.py does for
the one-shot step.  FOR INFORMATION: the test asserts with the r of tests/golden/train_full_gradient_ratios.json, which this
tool neither reads nor changes; a tensor over that r is a finding about accumulate()."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gradcheck as G                                   # noqa: E402
import accumulate_cases as A                            # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else A.RATIOS
    cases, worst, worst_at = {}, 0.0, None
    for case in A.CASES:
        cid = A.case_id(case)
        got, yard, loss, ref_loss, secs = A.run_case(case)
        print(f"{cid}: loss {loss:.5f} (oracle {ref_loss:.5f}), oracle + metrics {secs:.1f} s")
        print(G.describe(cid, got, yard), flush=True)
        cases[cid] = dict(G.ratios(got, yard), loss=loss, oracle_loss=ref_loss)
        for k in got:
            if got[k]["block"] > G.OWN_MARGIN:          # below the margin the bound holds for any r
                q = got[k]["block"] / max(yard[k]["block"], 1e-12)
                if q > worst:
                    worst, worst_at = q, f"{cid} {k}"
    doc = {"what": "block error of TrainStep.accumulate / block error of the bf16-autocast oracle, per tensor, against the fp32 "
                   "oracle (tests/gradcheck.py; train-mode BatchNorm: the per-chunk reference of tests/accumulate_ref.py); written "
                   "by tools/accumulate_gradient_ratios.py on an MI355X.  For information: tests/test_gpu_accumulate.py asserts "
                   "with the r of train_full_gradient_ratios.json.  measured_worst_ratio is taken over the tensors whose own "
                   "block error exceeds gradcheck.OWN_MARGIN (0.02), as there",
           "measured_worst_ratio": worst, "measured_worst_at": worst_at, "cases": cases}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("worst ratio", worst, worst_at)


if __name__ == "__main__":
    main()
