"""CPU tests of the six fp32 bounds files (tests/golden/{conv,token,head,optim,attn,act}_operator_bounds.json) and of the `check` the GPU sweeps hold
the kernels to with them (tests/operator_sweep.py).

What a bounds file must satisfy, on whichever machine the test runs:
  * structure: an entry for exactly the cases that have one of their own, and an operator summary that follows from the per-case figures;
  * regeneration on the machine the file was generated with (`generated_with` equals this machine's fingerprint): the same figures, to the
    printed precision;
  * regeneration anywhere else, or of a file without a fingerprint: the same keys, and every figure within FACTOR of the other side's
    yardstick in both directions -- e' <= FACTOR * max(e, m) and e <= FACTOR * max(e', m') with e, m the committed figure and operator
    median and e', m' the fresh ones.  FACTOR is the sweeps' own, for their own reason: another CPU's fp32 evaluation is another summation
    order of the same expression.  Where the committed yardstick is 0 (copies and single adds) the fresh figure is 0.
    The criterion is stated for the default thread set (1 and 4, largest figure), which is what runs here.
"""
import re
import statistics

import pytest
import torch

import operator_sweep as SW
from operator_sweep import FACTOR


@pytest.fixture(scope="module", params=SW.SUITES)
def suite_name(request):
    return request.param


@pytest.fixture(scope="module")
def committed(suite_name):
    return SW.load_bounds(suite_name)


@pytest.fixture(scope="module")
def fresh(suite_name):
    return SW.generate(suite_name)


def test_committed_file_has_an_entry_per_case_and_a_summary_that_follows_from_them(suite_name, committed):
    S = SW.suite(suite_name)
    assert set(committed) <= {"cases", "operators", "generated_with"}
    assert set(committed["cases"]) == {S.bounds_id(c) for c in S.BOUNDS_CASES}
    pools = {}
    for cid, qs in committed["cases"].items():
        for q, e in qs.items():
            pools.setdefault(S.BY_ID[cid]["op"], {}).setdefault(S.pool_key(q), []).append(e)
    assert {op: set(qs) for op, qs in pools.items()} == {op: set(qs) for op, qs in committed["operators"].items()}
    for op, qs in pools.items():
        for q, v in qs.items():
            got = committed["operators"][op][q]
            assert got["n"] == len(v) and got["worst"] == max(v), (op, q)
            # the median of an even count is a mean taken before the figures were rounded to four digits: one unit of the last one
            assert abs(got["median"] - statistics.median(v)) <= 1e-3 * statistics.median(v), (op, q, got["median"], statistics.median(v))


def test_regenerating_the_bounds_reproduces_the_committed_file(suite_name, committed, fresh):
    S = SW.suite(suite_name)
    if committed.get("generated_with") == SW.fingerprint():
        assert set(fresh["cases"]) == set(committed["cases"])
        for cid in sorted(fresh["cases"]):
            assert fresh["cases"][cid] == committed["cases"][cid], cid
        assert fresh["operators"] == committed["operators"]
        return
    assert set(fresh["cases"]) == set(committed["cases"])
    worst, misses = [0.0, 0.0], []
    for cid in sorted(fresh["cases"]):
        assert set(fresh["cases"][cid]) == set(committed["cases"][cid]), cid
        op = S.BY_ID[cid]["op"]
        for q, e1 in fresh["cases"][cid].items():
            e0 = committed["cases"][cid][q]
            y0 = max(e0, committed["operators"][op][S.pool_key(q)]["median"])
            y1 = max(e1, fresh["operators"][op][S.pool_key(q)]["median"])
            if y0 == 0:
                if e1 != 0:
                    misses.append(f"{cid} {q}: committed yardstick 0, fresh figure {e1:.4e}")
                continue
            worst = [max(worst[0], e1 / y0), max(worst[1], e0 / y1 if y1 else float("inf"))]
            if not (e1 <= FACTOR * y0 and e0 <= FACTOR * y1):
                misses.append(f"{cid} {q}: committed {e0:.4e} (yardstick {y0:.4e}), fresh {e1:.4e} (yardstick {y1:.4e})")
    print(f"{suite_name}: largest fresh figure {worst[0]:.2f} x the committed yardstick, largest committed figure {worst[1]:.2f} x the fresh yardstick "
          f"(committed with {committed.get('generated_with')}, here {SW.fingerprint()})")
    assert not misses, "\n  ".join(misses)


# ------------------------------------------------------------------------------------------------ `check` bites
BITE_CASES = {"conv": ("cbs-k3s1-2x5x9-4to12",), "token": ("addpos-c32", "mswsa-c64-dh32-mix"), "head": ("loss-base-nc3",),
              "optim": ("adamw-onecycle-n3076", "adamw-clipscale-n1020"), "attn": ("attn-t80-c24-dh8", "attn-peaked-t240-c64-dh32"), "act": ("act-mish", "unary-tanh_hw")}


def _check_kwargs(S, suite_name, case, ref, r32):
    if suite_name == "token":
        return dict(quantities=S.compared(case, ref), bit_equal={q: r32[q] for q in S.EXACT.get(case["op"], ())})
    return dict(discrete=S.EXACT) if suite_name == "head" else {}


@pytest.mark.parametrize("suite_name,cid", [(s, c) for s, cs in BITE_CASES.items() for c in cs])
def test_check_passes_the_float32_reference_and_refuses_what_it_must(suite_name, cid):
    """got = the reference in float32 on the CPU passes; a missing quantity, a NaN, an offset of 16 x the bound and a changed entry of a
    bit-equal / discrete quantity do not"""
    S, bounds = SW.suite(suite_name), SW.load_bounds(suite_name)
    case = S.BY_ID[cid]
    inp = S.make_inputs(case)
    ref, r32 = S.reference(case, inp, torch.float64), S.reference(case, inp, torch.float32)
    kw = _check_kwargs(S, suite_name, case, ref, r32)
    exact = set(kw.get("bit_equal", ())) | {q for q in kw.get("discrete", ()) if q in ref}
    got = {q: t.detach() for q, t in r32.items() if torch.is_tensor(t)}
    SW.check(S, case, got, ref, bounds, **kw)

    compared = kw.get("quantities") or S.float_quantities(ref)
    q = compared[0]
    with pytest.raises(AssertionError, match="produced no"):
        SW.check(S, case, {k: v for k, v in got.items() if k != q}, ref, bounds, **kw)
    bad = got[q].clone()
    bad.view(-1)[0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        SW.check(S, case, dict(got, **{q: bad}), ref, bounds, **kw)
    for q in (q for q in compared if q not in exact):        # one quantity at a time: the reference plus 16 x the bound, in the figure's units
        e32 = bounds["cases"][S.bounds_id(case)][q]
        tol = min(SW.project_bar(q), FACTOR * max(e32, bounds["operators"][case["op"]][S.pool_key(q)]["median"]))
        scale = 1.0 if "out:" in q else float(ref[q].abs().max())
        bad = ref[q].clone()
        bad.view(-1)[int(ref[q].abs().argmax())] += 16 * tol * scale
        assert tol > 0
        with pytest.raises(AssertionError, match=re.escape(q)):
            SW.check(S, case, dict(got, **{q: bad.to(got[q].dtype)}), ref, bounds, **kw)
    for q in sorted(exact):
        bad = got[q].clone()
        flat = bad.view(-1)
        flat[0] = ~flat[0] if bad.dtype == torch.bool else flat[0] + 1
        with pytest.raises(AssertionError, match=re.escape(q)):
            SW.check(S, case, dict(got, **{q: bad}), ref, bounds, **kw)
