"""Regenerate tests/golden/head_operator_bounds.json: the error of the YOLOX head references evaluated in float32 on the CPU against the
same expressions in float64, for every case of tests/head_cases.py that has float quantities (pred, loss, e2e).

    python tests/golden/make_head_bounds.py [--threads N[,N...]] [--out FILE]

CPU only.  tests/test_head_operators.py holds the HIP kernels to FACTOR x max(e32 of the case, median e32 of the operator) per quantity
(capped by the project's bars), so the figures here are the yardstick: they come from the reference alone, never from the kernels.
The fp32 sums of torch's CPU kernels move a little with the thread count; with several --threads values (default 1 and 4) every figure
is the LARGEST over them.

File layout: {"cases": {case id: {quantity: e32}}, "operators": {operator: {quantity: {"median": .., "worst": .., "n": ..}}}}; "out:"
quantities are absolute errors of O(1) tensors, everything else is relative to the reference tensor's max-norm.
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import head_cases as HC  # noqa: E402

OUT = os.path.join(HERE, "head_operator_bounds.json")


def evaluate(threads):
    torch.set_num_threads(threads)
    cases = {}
    for case in HC.FLOAT_CASES:
        inp = HC.make_inputs(case)
        r64, r32 = HC.reference(case, inp, torch.float64), HC.reference(case, inp, torch.float32)
        qs = HC.float_quantities(r64)
        assert qs == HC.float_quantities(r32)
        for q in HC.EXACT:      # the figures mean something only where both precisions reach the same assignment
            assert q not in r64 or torch.equal(r64[q], r32[q]), (case["id"], q)
        cases[case["id"]] = {q: HC.measure(q, r32[q], r64[q])[0] for q in qs}
    return cases


def summarise(cases):
    pools = {}
    for cid, qs in cases.items():
        for q, e in qs.items():
            pools.setdefault(HC.BY_ID[cid]["op"], {}).setdefault(HC.pool_key(q), []).append(e)
    return {op: {q: {"median": statistics.median(v), "worst": max(v), "n": len(v)} for q, v in sorted(qs.items())} for op, qs in sorted(pools.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", default="1,4")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    runs = [evaluate(int(t)) for t in a.threads.split(",")]
    cases = {cid: {q: max(r[cid][q] for r in runs) for q in runs[0][cid]} for cid in runs[0]}
    doc = {"cases": cases, "operators": summarise(cases)}
    doc = json.loads(json.dumps(doc), parse_float=lambda s: float(f"{float(s):.4e}"))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    worst_out = max(v["worst"] for qs in doc["operators"].values() for q, v in qs.items() if "out:" in q)
    worst_rel = max(v["worst"] for qs in doc["operators"].values() for q, v in qs.items() if "out:" not in q)
    print(f"{len(cases)} cases -> {a.out}: worst fp32 absolute error {worst_out:.2e} (bar {HC.FWD_ATOL:.0e}), "
          f"worst fp32 error relative to the max-norm {worst_rel:.2e} (bar {HC.GRAD_RTOL:.0e})")


if __name__ == "__main__":
    main()
