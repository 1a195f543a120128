"""Regenerate tests/golden/{conv,token,head,optim,attn,act}_operator_bounds.json: the error of a suite's reference expressions evaluated in float32 on
the CPU against the same expressions in float64, for every case of tests/{conv,token,head,optim,attn,act}_cases.py that has a bounds entry of its
own (head: the cases with float quantities -- pred, loss, e2e; token, attn: not the cases that rerun another case's arithmetic under a knob).

    python tests/golden/make_operator_bounds.py conv|token|head|optim|attn|act [--threads N[,N...]] [--out FILE]

CPU only.  tests/test_{conv,token,head,optim,attn,act}_operators.py hold the HIP kernels to FACTOR x max(e32 of the case, median e32 of the operator) per
quantity (capped by the project's bars), so the figures here are the yardstick: they come from the reference alone, never from the kernels.
The fp32 sums of torch's CPU kernels move a little with the thread count; with several --threads values (default 1 and 4) every figure
is the LARGEST over them.  They move with the CPU and the torch build as well, so the file records what it was generated with, and
tests/test_operator_bounds.py says what a file must satisfy where it is regenerated on another machine.

File layout: {"cases": {case id: {quantity: e32}}, "operators": {operator: {quantity: {"median": .., "worst": .., "n": ..}}},
"generated_with": {..}}; "out:" quantities are absolute errors of O(1) tensors, everything else is relative to the reference tensor's
max-norm.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import operator_sweep as SW  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("suite", choices=SW.SUITES)
    ap.add_argument("--threads", default="1,4")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = a.out or SW.bounds_path(a.suite)
    doc = SW.generate(a.suite, [int(t) for t in a.threads.split(",")])
    SW.write_bounds(doc, out)
    worst_out = max((v["worst"] for qs in doc["operators"].values() for q, v in qs.items() if "out:" in q), default=0.0)      # (optim: no "out:" quantity)
    worst_rel = max((v["worst"] for qs in doc["operators"].values() for q, v in qs.items() if "out:" not in q), default=0.0)      # (act: only "out:" quantities)
    print(f"{len(doc['cases'])} cases -> {out}: worst fp32 absolute error {worst_out:.2e} (bar {SW.FWD_ATOL:.0e}), "
          f"worst fp32 error relative to the max-norm {worst_rel:.2e} (bar {SW.GRAD_RTOL:.0e})")


if __name__ == "__main__":
    main()
