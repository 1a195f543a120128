"""CPU tests of the non-finite sweep's own instrument (no GPU, no library): for every recipe of tests/nonfinite_cases.py the element sets
derived from the float64 reference are what the recipe says they are, they are consistent with the reference's own NaN run, and the
zero-weighted set is empty outside the declared caps -- so that a recipe cannot quietly become empty or turn permissive."""
import pytest
import torch

import nonfinite_cases as NC

RECIPE_IDS = [r["id"] for r in NC.ALL_RECIPES]

STATEMENTS = {
    "I-is": lambda I, D, arg: torch.equal(I, arg),
    "I-covers": lambda I, D, arg: bool(arg.any()) and bool(I[arg].all()),
    "I-all": lambda I, D, arg: I.numel() > 0 and bool(I.all()),
    "D-all": lambda I, D, arg: D.numel() > 0 and bool(D.all()),
    "D-some": lambda I, D, arg: bool(D.any()),
    "D-within": lambda I, D, arg: bool(D.any()) and not bool((D & ~arg).any()),
}


def test_recipe_table_is_the_one_the_sweep_is_about():
    assert len(NC.CONV_RECIPES) == 14 and len(NC.TOKEN_RECIPES) == 18
    assert sorted(NC.PART240) == ["mswsa-c64-dh32-part240", "mswsa-c64-dh32-part240-peaked"]
    either = {r["id"]: r["caps"] for r in NC.ALL_RECIPES if r["zero"] == "either"}
    assert either == {"lstm-c48-none@sample1": NC.LSTM_NONE_CAPS, "lstm-c256-none-lstmtile@sample1": NC.LSTM_NONE_CAPS,
                      "cbsdw-k3s2-2x5x9-256@pixel": {"eval/grad:w": 5.0 / 9.0}}
    assert all(r["zero"] == "must_be_clean" and not r["caps"] for r in NC.ALL_RECIPES if r["id"] not in either)
    assert all(NC.case_of(r)["op"] in NC.TC.MSWSA_OPS for r in NC.ALL_RECIPES if r["where"] == "unkept")


@pytest.mark.parametrize("rid", RECIPE_IDS)
def test_poisoned_inputs_differ_from_the_case_only_on_P(rid):
    recipe = NC.BY_ID[rid]
    inp = NC.SUITES[recipe["suite"]].make_inputs(NC.case_of(recipe))
    m = NC.poison_mask(recipe, inp)
    assert 0 < int(m.sum()) and (recipe["where"] == "masked" or int(m.sum()) < m.numel() or NC.case_of(recipe)["B"] == 1)
    for fill, test in ((0.0, lambda t: t == 0), ("randn", torch.isfinite), (float("nan"), torch.isnan), (float("inf"), torch.isposinf)):
        p = NC.poisoned(recipe, inp, fill)
        assert sorted(p) == sorted(inp) and all(p[k] is inp[k] for k in inp if k != recipe["key"])
        x = p[recipe["key"]]
        assert bool(test(x[m]).all()) and torch.equal(x[~m], inp[recipe["key"]][~m])
    a, b = NC.poisoned(recipe, inp, "randn")["x"][m], NC.poisoned(recipe, inp, "randn")["x"][m]
    assert torch.equal(a, b) and float(a.abs().max()) > 1.0          # seeded by the recipe id; a fill that moves results


@pytest.mark.parametrize("rid", RECIPE_IDS)
def test_element_sets_of_the_float64_reference(rid):
    recipe = NC.BY_ID[rid]
    _inp, r0, sets, rN = NC.derive(recipe)
    assert sorted(sets) == sorted(r0) == sorted(rN)
    for q, (I, D, A) in sets.items():
        assert bool(torch.isfinite(r0[q]).all()), q
        bad = ~torch.isfinite(rN[q])
        # the three runs agree: what moved under a finite fill is non-finite under NaN (I and D cover everything), rN is finite on
        # I \ A and non-finite on D
        assert bool((I | D).all()) and not bool((I & D).any()), (q, int((~(I | D)).sum()))
        assert not bool(bad[I & ~A].any()) and bool(bad[D].all()), q
        cap = recipe["caps"].get(q, 0.0)
        print(f"{rid:44s} {q:22s} I {NC.share(I):.4f}  D {NC.share(D):.4f}  A {NC.share(A):.4f}  cap {cap:.4f}")
        if recipe["zero"] == "either":
            assert NC.share(A) <= cap + 1e-12, (q, NC.share(A), cap)
            assert cap == 0.0 or NC.share(A) == pytest.approx(cap, abs=1e-12), (q, NC.share(A), cap)     # a cap is the share, not slack over it
            assert not bool((NC.clean_set(recipe, q, sets) & bad).any())
        else:
            assert not recipe["caps"]
            assert recipe["where"] == "unkept" or NC.share(A) == 0.0, (q, NC.share(A))
    assert set(recipe["caps"]) <= set(sets)
    said = NC.expect(recipe)
    assert said and {q for q, _s, _a in said} <= set(sets), [q for q, _s, _a in said if q not in sets]
    for q, statement, arg in said:
        I, D, _A = sets[q]
        assert arg is None or arg.shape == I.shape, (q, statement)
        assert STATEMENTS[statement](I, D, arg), (rid, q, statement, NC.share(I), NC.share(D))
    # every recipe has something to contain and something to propagate (mask token: nothing may depend on a masked row)
    assert any(bool(NC.clean_set(recipe, q, sets).any()) for q in sets)
    assert recipe["where"] == "masked" or any(bool(D.any()) for _I, D, _A in sets.values())
