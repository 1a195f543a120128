"""Regenerate tests/golden/token_operator_bounds.json: the error of the token-path operators' reference expression evaluated in float32
on the CPU against the same expression in float64, for every case of tests/token_cases.py.

    python tests/golden/make_token_bounds.py [--threads N[,N...]] [--out FILE]

CPU only.  tests/test_token_operators.py holds the HIP kernels to FACTOR x max(e32 of the case, median e32 of the operator) per quantity
(capped by the project's bars), so the figures here are the yardstick: they come from the reference alone, never from the kernels.
The fp32 sums of torch's CPU kernels move a little with the thread count; with several --threads values (default 1 and 4) every figure
is the LARGEST over them.

File layout: {"cases": {case id: {quantity: e32}}, "operators": {operator: {quantity: {"median": .., "worst": .., "n": ..}}}}; outputs
("out:") are absolute errors of O(1) tensors, everything else is relative to the reference tensor's max-norm.
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

import token_cases as TC  # noqa: E402

OUT = os.path.join(HERE, "token_operator_bounds.json")


def evaluate(threads):
    torch.set_num_threads(threads)
    cases = {}
    for case in TC.ALL_CASES:
        if TC.bounds_id(case) != case["id"]:
            continue
        inp = TC.make_inputs(case)
        r64, r32 = TC.reference(case, inp, torch.float64), TC.reference(case, inp, torch.float32)
        assert r64.keys() == r32.keys()
        cases[case["id"]] = {q: TC.measure(q, r32[q], r64[q])[0] for q in sorted(r64)}
    return cases


def summarise(cases):
    pools = {}
    for cid, qs in cases.items():
        for q, e in qs.items():
            pools.setdefault(TC.BY_ID[cid]["op"], {}).setdefault(TC.pool_key(q), []).append(e)
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
    print(f"{len(cases)} cases -> {a.out}: worst fp32 output error {worst_out:.2e} (bar {TC.FWD_ATOL:.0e}), "
          f"worst fp32 gradient / score error {worst_rel:.2e} of the max-norm (bar {TC.GRAD_RTOL:.0e})")


if __name__ == "__main__":
    main()
