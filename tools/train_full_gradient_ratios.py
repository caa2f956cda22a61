"""Measure r of tests/test_gpu_train_full.py on an MI355X:

    python tools/train_full_gradient_ratios.py [out.json]        # default: tests/golden/train_full_gradient_ratios.json

Runs that test's cases (tests/train_full_cases.py) once (one TrainStep forward / backward each; the fp32 oracle's autograd as
the reference, the oracle under bf16 autocast as the yardstick) and writes, per case and tensor class, the distribution of
`block error of TrainStep / block error of the yardstick` (median, p90, worst, name of the worst), and r = 1.25 x the worst
ratio among the tensors whose own block error exceeds the bound's additive margin (gradcheck.OWN_MARGIN: below it
block error <= r x yardstick + margin holds for any r), capped at 2.
A tensor that needs more than 2 is a finding, not a reason to raise the cap (tests/gradcheck.py::R_MAX)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gradcheck as G                                   # noqa: E402
import train_full_cases as T                            # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.RATIOS
    cases, worst, worst_at = {}, 0.0, None
    for case in T.CASES:
        cid = T.case_id(case)
        got, yard, loss, ref_loss, secs = T.run_case(case)
        print(f"{cid}: loss {loss:.5f} (oracle {ref_loss:.5f}), oracle + metrics {secs:.1f} s")
        print(G.describe(cid, got, yard), flush=True)
        cases[cid] = G.ratios(got, yard)
        for k in got:
            if got[k]["block"] > G.OWN_MARGIN:          # below the margin the bound holds for any r
                q = got[k]["block"] / max(yard[k]["block"], 1e-12)
                if q > worst:
                    worst, worst_at = q, f"{cid} {k}"
        for line in G.violations(got, yard, G.R_MAX):
            print("  over r = 2:", line)
    doc = {"what": "block error of TrainStep / block error of the bf16-autocast oracle, per tensor, against the fp32 oracle "
                   "(tests/gradcheck.py); written by tools/train_full_gradient_ratios.py on an MI355X.  measured_worst_ratio is "
                   "the largest ratio among the tensors whose own block error exceeds gradcheck.OWN_MARGIN (0.02): below that "
                   "margin the asserted bound, block error <= r x yardstick + 0.02, holds for any r.  The per-class figures "
                   "under 'cases' cover every tensor; the 'scalar' class is logit_scale, one number made of cancelling terms "
                   "whose yardstick can land arbitrarily near zero (ratios of 7 and 66 at absolute errors of 0.017 and 0.004)",
           "measured_worst_ratio": worst, "measured_worst_at": worst_at, "r": min(G.R_MAX, 1.25 * worst), "cases": cases}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("r =", doc["r"], "from", worst, worst_at)


if __name__ == "__main__":
    main()
