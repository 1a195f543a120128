"""The recipes of the non-finite sweep (tests/test_nonfinite_operators.py): which results of an operator may depend on a poisoned part
of its input, derived from the float64 references of the conv and token suites.  CPU only: nothing here imports the library.

A recipe is an existing case of tests/conv_cases.py or tests/token_cases.py, the input to poison and the elements P of it:
  last      all of the last sample of x (conv cases)
  pixel     the last pixel (H - 1, W - 1) of sample 0, all channels
  sample1   sample 1 of x (ConvLSTM)
  unkept    the rows of x that `kept_slots(case)` does not keep, the dropped window included (MS-WSA)
  masked    x at the masked positions (mask token)
`derive(recipe)` evaluates the case's own `reference(case, inp, torch.float64)` with P := 0 (r0), P := 3 randn from a generator seeded by
the recipe id (r1) and P := NaN (rN) and returns, per quantity, three element sets:
  I   independent    r0 == r1 element by element: two finite fills with the same float64 result, the result does not depend on P
  D   dependent      r0 != r1 and rN not finite
  A   zero-weighted  I and rN not finite: the reference itself multiplies the poison by zero there
What a recipe asks of the device on A is its `zero` field: "must_be_clean" (clean on all of I whatever rN says: the compact MS-WSA form
promises that unselected tokens are never read; the reference's dense formulation with masks does not decide) or "either" (clean or
non-finite on A, with the share of A per quantity capped by `caps`; clean on I \\ A).  Every quantity without a cap has an empty A.
Three recipes are "either": the two ConvLSTM ones without a state (the weight-gradient rows of the skipped forget gate and of the absent h
half: 0.25 of d b, 0.625 of d w) and the pixel recipe of the depth-wise stride-2 conv (5 / 9 of the eval-mode d w: PIXEL_OPTIONS below).

`expect(recipe)` states what the sets must look like, as (quantity, statement, argument) conditions that tests/test_nonfinite_reference.py
asserts, so that a recipe cannot quietly become empty:
  I-is      I equals the given mask                       I-covers  I holds the given mask (it may hold more: elements no tap reaches)
  I-all     every element is independent                   D-all     every element is dependent
  D-some    some element is dependent                      D-within  D lies inside the given mask and is not empty
"""
import torch

import conv_cases as CC
import operator_sweep as SW
import token_cases as TC

SUITES = {"conv": CC, "token": TC}
POISONS = {"nan": float("nan"), "inf": float("inf")}


def _recipe(suite, cid, where, zero="must_be_clean", caps=None, table=False):
    assert cid in SUITES[suite].BY_ID, cid
    return dict(id=f"{cid}@{where}", suite=suite, case=cid, key="x", where=where, zero=zero, caps=caps or {}, table=table)


TABLE_CBS = ("cbs-k3s1-2x5x9-4to12", "cbs-k1s1-2x5x9-32to36-src12", "cbsdw-k3s2-2x5x9-256")
PART240 = [c["id"] for c in TC.PART_CASES if c["T"] == 240 and c["C"] == 64]
LSTM_NONE_CAPS = {"grad:b": 0.25, "grad:w": 0.625}      # the forget gate (no c0); that and the h half of the reduction (no h0)
# The depth-wise 3x3 stride-2 conv on a 5 x 9 map: the last pixel is read by ONE output, (2, 4), whose window covers rows 3..5 and columns
# 7..9.  Row 5 and column 9 are zero padding, so five of the nine taps of every channel's weight gradient are (non-finite dz) x (padding
# 0) in the reference itself, and nothing else reaches them: a zero-weighted share of 5 / 9 by the geometry, in the eval-mode dW only
# (a dense conv sums over input channels and outputs whose other taps see the pixel, batch statistics reach everything).
PIXEL_OPTIONS = {"cbsdw-k3s2-2x5x9-256": dict(zero="either", caps={"eval/grad:w": 5.0 / 9.0})}

CONV_RECIPES = (
    [_recipe("conv", c, "last", table=True) for c in TABLE_CBS]
    + [_recipe("conv", c, "last") for c in ("cbs-k3s2-2x5x9-32to36", "cbs-k3s4-2x5x9-12to16", "cbs-k1s2-2x5x9-4to12", "cbsdw-k3s1-2x5x9-4")]
    + [_recipe("conv", "down-f2o-3x12x28-20to48", "last", table=True), _recipe("conv", "down-f4n-3x13x30-4to64-pe", "last"),
       _recipe("conv", "dwconv-k7-1x7x3-64", "last", table=True), _recipe("conv", "dwconv-k3-2x5x9-64-win32of128", "last")]
    + [_recipe("conv", c, "pixel", **PIXEL_OPTIONS.get(c, {})) for c in TABLE_CBS])
TOKEN_RECIPES = (
    [_recipe("token", c, "unkept", table=True) for c in ("mswsa-c64-dh32-mix", "mswsa-c48-dh24-mix-cb", "mswsa-c48-dh24-mix-drop", "mswsa-c64-dh32-part80")]
    + [_recipe("token", c, "unkept") for c in ("mswsa-c64-dh32-mix-fused", "mswsa-c64-dh32-mix-fused-nograd", "mswsa-c64-dh8-mix", "mswsa-c96-dh16-mix",
                                               "mswsa-c32-dh32-empty2", "mswsa-c64-dh32-part80-fused")]
    + [_recipe("token", c, "unkept") for c in PART240]
    + [_recipe("token", "lstm-c48-given", "sample1", table=True),
       _recipe("token", "lstm-c48-none", "sample1", zero="either", caps=LSTM_NONE_CAPS, table=True),
       _recipe("token", "lstm-c256-given-two-drop", "sample1"),
       _recipe("token", "lstm-c256-none-lstmtile", "sample1", zero="either", caps=LSTM_NONE_CAPS)]
    + [_recipe("token", "masktoken-c48-every257", "masked", table=True), _recipe("token", "masktoken-c1024-all-nope", "masked")])
ALL_RECIPES = CONV_RECIPES + TOKEN_RECIPES
BY_ID = {r["id"]: r for r in ALL_RECIPES}
assert len(BY_ID) == len(ALL_RECIPES), "duplicate recipe ids"


def case_of(recipe):
    return SUITES[recipe["suite"]].BY_ID[recipe["case"]]


# ------------------------------------------------------------------------------------------------ the poisoned elements
def kept_rows(case):
    """[NW, T] bool: the rows of a MS-WSA case that its selection keeps"""
    m = torch.zeros(case["B"] * case["N"], case["T"], dtype=torch.bool)
    for w, slots in TC.kept_slots(case).items():
        m[w, slots] = True
    return m


def poison_mask(recipe, inp):
    """bool, the shape of inp[key]: the elements P"""
    case, x = case_of(recipe), inp[recipe["key"]]
    m = torch.zeros(x.shape, dtype=torch.bool)
    where = recipe["where"]
    if where == "last":
        m[-1] = True
    elif where == "pixel":
        m[0, -1, -1] = True
    elif where == "sample1":
        m[1] = True
    elif where == "unkept":
        m[~kept_rows(case)] = True
    elif where == "masked":
        m[TC.token_mask(case)] = True
    else:
        raise KeyError(where)
    assert bool(m.any()) and x.dtype == torch.float32, recipe["id"]
    return m


def poisoned(recipe, inp, fill):
    """a copy of the inputs with P := fill ("randn": 3 randn from the recipe's generator, else a number)"""
    out = dict(inp)
    x, m = inp[recipe["key"]].clone(), poison_mask(recipe, inp)
    if fill == "randn":
        x[m] = 3.0 * torch.randn(int(m.sum()), generator=SW.gen("poison-" + recipe["id"]))
    else:
        x[m] = float(fill)
    out[recipe["key"]] = x
    return out


# ------------------------------------------------------------------------------------------------ the element sets
_DERIVED = {}


def derive(recipe):
    """(inputs of the case, r0, {quantity: (I, D, A)}, rN), evaluated once per recipe and never written to"""
    if recipe["id"] not in _DERIVED:
        S, case = SUITES[recipe["suite"]], case_of(recipe)
        inp = S.make_inputs(case)
        r0, r1, rN = (S.reference(case, poisoned(recipe, inp, fill), torch.float64) for fill in (0.0, "randn", float("nan")))
        sets = {}
        for q in S.float_quantities(r0):
            indep, bad = r0[q] == r1[q], ~torch.isfinite(rN[q])
            sets[q] = (indep, ~indep & bad, indep & bad)
        _DERIVED[recipe["id"]] = (inp, r0, sets, rN)
    return _DERIVED[recipe["id"]]


def clean_set(recipe, q, sets):
    """where the device must be finite and equal to its zero-filled run"""
    indep, _dep, zw = sets[q]
    return indep & ~zw if recipe["zero"] == "either" else indep


def share(mask):
    return float(mask.double().mean()) if mask.numel() else 0.0


# ------------------------------------------------------------------------------------------------ what the sets must look like
def _mode_q(case, *names):
    return [(mode, f"{mode}/{n}") for mode in case["modes"] for n in names]


def _reach(case, py, px):
    """[Ho, Wo] bool: the outputs of the case's conv that read input pixel (py, px)"""
    k, s = case["k"], case["s"]
    Ho, Wo = CC.conv_hw(case["H"], case["W"], k, s)
    p = (k - 1) // 2
    m = torch.zeros(Ho, Wo, dtype=torch.bool)
    for oy in range(Ho):
        for ox in range(Wo):
            m[oy, ox] = 0 <= py - (oy * s - p) < k and 0 <= px - (ox * s - p) < k
    return m


def expect(recipe):
    case, inp, out = case_of(recipe), SUITES[recipe["suite"]].make_inputs(case_of(recipe)), []
    op, where, exact = case["op"], recipe["where"], "I-is" if recipe["table"] else "I-covers"

    def others(q_shape, sample):      # every sample but `sample`
        m = torch.ones(q_shape, dtype=torch.bool)
        m[sample] = False
        return m

    if op in ("cbs", "cbs_dw") and where == "last":
        Ho, Wo = CC.conv_hw(case["H"], case["W"], case["k"], case["s"])
        shapes = {"out:y": (case["B"], Ho, Wo, case["cout"]), "grad:x": tuple(inp["x"].shape)}
        if "x2" in inp:
            shapes["grad:x2"] = tuple(inp["x2"].shape)
        params = ("grad:w", "grad:bn_w", "grad:bn_b")
        for mode in case["modes"]:
            if mode == "train":      # batch statistics reach every row
                qs = ["out:y", "stat:run_mean", "stat:run_var", *shapes, *params]
                out += [(f"train/{n}", "D-all" if recipe["table"] else "D-some", None) for n in dict.fromkeys(qs)]
                continue
            for n, shp in shapes.items():
                if mode == "infer" and n != "out:y":
                    continue
                out.append((f"{mode}/{n}", exact, others(shp, -1)))
            if mode == "eval":
                out += [(f"eval/{n}", "D-all" if recipe["table"] else "D-some", None) for n in params]
    elif op in ("cbs", "cbs_dw") and where == "pixel":
        Ho, Wo = CC.conv_hw(case["H"], case["W"], case["k"], case["s"])
        near = torch.zeros(case["B"], Ho, Wo, case["cout"], dtype=torch.bool)
        near[0][_reach(case, case["H"] - 1, case["W"] - 1)] = True
        assert 1 <= int(near[0, :, :, 0].sum()) <= 4
        for mode in case["modes"]:
            if mode == "train":
                out.append(("train/out:y", "D-some", None))
                continue
            out.append((f"{mode}/out:y", "D-within", near))
            out.append((f"{mode}/out:y", "I-covers", ~near))      # sample 1 and everything of sample 0 outside the neighbourhood
            if mode == "eval":
                out.append(("eval/grad:x", "I-covers", others(tuple(inp["x"].shape), 0)))
    elif op == "down":
        f = case["f"]
        y_shape = (case["B"], case["H"] // f, case["W"] // f, case["cout"])
        out += [("train/out:y", "I-is", others(y_shape, -1)), ("train/grad:x", exact, others(tuple(inp["x"].shape), -1)),
                ("train/grad:ln_b", "I-all", None), ("train/grad:ln_w", "D-all", None), ("train/grad:w", "D-all", None)]
    elif op == "dwconv":
        if case["B"] == 1:
            out += [("train/grad:x", "I-all", None), ("train/grad:b", "I-all", None), ("train/out:y", "D-all", None)]
        else:
            out += [("train/grad:x", "I-all", None), ("train/grad:b", "I-all", None), ("train/out:y", "I-is", others(tuple(inp["x"].shape), -1)),
                    ("train/grad:w", "D-some", None)]
    elif op == "lstm":
        state = [n for n in ("h0", "c0") if n in inp]
        out += [(q, "I-is", others(tuple(inp["x"].shape), 1)) for q in ["out:h1", "out:c1", "grad:x"] + [f"grad:{n}" for n in state]]
        if recipe["zero"] == "either":
            out += [("grad:w", "D-some", None), ("grad:b", "D-some", None)]
        else:
            out += [("grad:w", "D-all", None), ("grad:b", "D-all", None)]
    elif op == "mask_token":
        out += [(q, "I-all", None) for q in ("out:y", "grad:x", "grad:token")]
    elif op in TC.MSWSA_OPS:
        kept = kept_rows(case)[..., None].expand(-1, -1, case["C"])
        out.append(("out:y", "I-is", kept))
        if not case["nograd"]:
            out.append(("grad:x", "I-is", kept))
            out += [(f"grad:{n}", "I-all", None) for n in inp if n not in TC.NO_GRAD and n not in ("x", "ln1_w")]
    else:
        raise KeyError(op)
    return out
