"""CPU tests of the elementwise sweep's own instruments (no GPU): the case table and the points of tests/act_cases.py, the float32
reference under `check`, and that `check` with the committed bounds (tests/golden/act_operator_bounds.json) bites: it passes a float32
restatement of the formulas of csrc/common.cuh (torch's exp and division in place of v_exp_f32 and v_rcp_f32) and refuses the same
restatement with one planted fault at a time (tests/test_operator_bounds.py regenerates the bounds file).
"""
import pytest
import torch

import act_cases as AC
import operator_sweep as SW

bounds = SW.bounds_fixture("act")

SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


# ------------------------------------------------------------------------------------------------ csrc/common.cuh in float32 torch
def restate(case, g, fault=None):
    """(y, dy or None): glu_act / glu_act_grad / the helpers as common.cuh writes them, in float32.  `fault`: one planted defect."""
    assert g.dtype == torch.float32
    one, zero = torch.ones_like(g), torch.zeros_like(g)
    f = lambda v: torch.full_like(g, v)      # noqa: E731

    def exp(x):
        return torch.exp(x) * f(1 + 2.0 ** -16) if fault == "tanh_exp_2^-16" else torch.exp(x)

    def sigmoid(x):
        return 1 / (1 + torch.exp(-x))

    def tanh(x):
        return 1 - 2 / (1 + exp(2 * x))

    def softplus(x):
        sp = torch.log1p(torch.exp(x))
        return sp if fault == "mish_no_threshold" else torch.where(x > 20, x, sp)

    def dsoftplus(x):       # e / (1 + e): the chain-rule factor of a derivative taken through softplus (inf / inf where e^x overflows)
        e = torch.exp(x)
        return e / (1 + e) if fault == "mish_no_threshold" else torch.where(x > 20, one, e / (1 + e))

    def erf(x):
        ax = x.abs()
        t = 1 / (0.3275911 * ax + 1)
        p = 1.061405429 * t - 1.453152027
        for c in (1.421413741, -0.284496736, 0.254829592):
            p = p * t + c
        return torch.copysign(1 - p * t * torch.exp(-ax * ax), x)

    def gelu(x):
        return 0.5 * x * (1 + erf(x * 0.70710678118654752440))

    def gelu_grad(x):
        return 0.5 * (1 + erf(x * 0.70710678118654752440)) + x * (0.39894228040143267794 * torch.exp(-0.5 * x * x))

    fn = case["fn"]
    if case["op"] == "unary":
        return {"sigmoid_hw": sigmoid, "tanh_hw": tanh, "gelu_erf": gelu, "gelu_erf_grad": gelu_grad, "softplus_t20": softplus,
                "rsqrt_hw": torch.rsqrt, "silu": lambda x: x * sigmoid(x)}[fn](g), None
    pos = g > 0
    alpha = SELU_ALPHA + (1e-5 if fault == "selu_alpha_6th_digit" else 0.0)
    relu6 = lambda x: torch.clamp(x, 0.0, 6.0)      # noqa: E731
    if fn == "gelu":
        return gelu(g), gelu_grad(g)
    if fn == "relu":
        return torch.clamp(g, min=0.0), torch.where(g >= 0 if fault == "relu_grad_1_at_0" else pos, one, zero)
    if fn == "silu":
        s = sigmoid(g)
        return g * s, s * (1 + g * (1 - s))
    if fn == "sigmoid":
        s = sigmoid(g)
        return s, s * (1 - s)
    if fn == "tanh":
        t = tanh(g)
        return t, 1 - t * t
    if fn == "mish":
        t = tanh(softplus(g))
        if fault == "mish_no_threshold":
            return g * t, t + g * (1 - t * t) * dsoftplus(g)
        return g * t, t + g * (1 - t * t) * (1 / (1 + torch.exp(-g)))
    if fn == "relu6":
        return relu6(g), torch.where(pos & ((g <= 6) if fault == "relu6_grad_1_at_6" else (g < 6)), one, zero)
    if fn == "leaky_relu":
        return torch.where(pos, g, f(0.01) * g), torch.where(pos, one, f(0.01))
    if fn == "elu":
        return torch.where(pos, g, torch.expm1(g)), torch.where(pos, one, torch.exp(g))
    if fn == "selu":
        return f(SELU_SCALE) * torch.where(pos, g, f(alpha) * torch.expm1(g)), torch.where(pos, f(SELU_SCALE), f(SELU_SCALE) * f(alpha) * torch.exp(g))
    if fn == "hard_sigmoid":
        return relu6(g + 3) / 6, torch.where((g > -3) & (g < 3), f(1.0) / f(6.0), zero)
    if fn == "hard_swish":
        upper = (g <= 3) if fault == "hard_swish_le_at_3" else (g < 3)
        return g * relu6(g + 3) / 6, torch.where(g <= -3, zero, torch.where(upper, g / 3 + 0.5, one))
    if fn == "hard_mish":
        return 0.5 * g * torch.clamp(g + 2, 0.0, 2.0), torch.where(g < -2, zero, torch.where(g <= 0, g + 1, one))
    if fn == "prelu":
        return torch.where(pos, g, f(case["slope"]) * g), torch.where(pos, one, f(case["slope"]))
    raise KeyError(fn)


def _run_check(case, got_of, bounds):
    inp = AC.make_inputs(case)
    ref, r32 = AC.reference(case, inp, torch.float64), AC.reference(case, inp, torch.float32)
    SW.check(AC, case, got_of(case, inp, r32), ref, bounds, bit_equal=AC.bit_equal(case, r32))


# ------------------------------------------------------------------------------------------------ the case table and the points
def test_case_table_covers_every_activation_code_every_helper_and_every_kink():
    from sast_amd.functional import GLU_ACTIVATIONS
    assert set(GLU_ACTIVATIONS.values()) == set(range(14)) == {c["code"] for c in AC.ACT_CASES}
    for c in AC.ACT_CASES:
        assert GLU_ACTIVATIONS[c["fn"]] == c["code"] and c["op"] == "act", c["id"]
    assert len(AC.ACT_CASES) == 14 and [c["code"] for c in AC.UNARY_CASES] == list(range(7)) and all(c["op"] == "unary" for c in AC.UNARY_CASES)
    assert AC.BY_ID["act-prelu"]["slope"] == 0.3 and all(c["slope"] == 0.0 for c in AC.ALL_CASES if c["fn"] != "prelu")
    assert {k for ks in AC.KINKS.values() for k in ks} | {2.0} == set(AC.ALL_KINKS) == {0.0, 2.0, -2.0, 3.0, -3.0, 6.0, 20.0}
    assert set(AC.PIECEWISE) <= set(AC.KINKS) and set(AC.KINKS) <= set(AC.ACT_CODES)
    g, kink = AC.points()
    assert g.dtype == torch.float32 and torch.equal(g[kink], AC.kink_points()) and int(kink.sum()) == 63
    grid = set((torch.arange(-24 * 1024, 24 * 1024 + 1, dtype=torch.float64) / 1024).tolist())
    assert grid <= set(g.double().tolist()) and set(AC.ALL_KINKS) <= grid
    for k in AC.ALL_KINKS:      # the neighbours are the adjacent fp32 values, in order
        near = AC.kink_points()[(AC.kink_points().double() - k).abs() <= 1e-5]
        assert near.numel() == 9 and float(near[4]) == k and bool((near[1:] > near[:-1]).all())
        assert torch.equal(torch.nextafter(near[:-1], torch.tensor(float("inf"))), near[1:]), k


@pytest.mark.parametrize("case", AC.ALL_CASES, ids=SW.ids(AC.ALL_CASES))
def test_input_conditions_hold(case):
    AC.check_conditions(case, AC.make_inputs(case))


def test_reference_states_the_conventions_at_the_kinks():
    """torch's derivative on the kink itself, which the float64 reference hands to `check`"""
    want = {"relu": {0.0: 0.0}, "relu6": {0.0: 0.0, 6.0: 0.0}, "leaky_relu": {0.0: 0.01}, "prelu": {0.0: 0.3}, "hard_sigmoid": {-3.0: 0.0, 3.0: 0.0},
            "hard_swish": {-3.0: 0.0, 3.0: 1.0}, "hard_mish": {-2.0: -1.0, 0.0: 1.0}, "elu": {0.0: 1.0}, "selu": {0.0: SELU_SCALE * SELU_ALPHA}}
    for name, at in want.items():
        case = AC.BY_ID[f"act-{name}"]
        for k, d in at.items():
            _y, dy = AC.evaluate_reference(case, torch.tensor([k], dtype=torch.float64))
            d = float(torch.tensor(d, dtype=torch.float32)) if name == "prelu" else d       # the slope is an fp32 parameter
            assert abs(float(dy) - d) < 1e-15, (name, k, float(dy))


def test_bounds_hold_every_quantity_and_stay_inside_the_project_bar(bounds):
    for case in AC.ALL_CASES:
        entry = bounds["cases"][case["id"]]
        assert set(entry) == set(AC.QUANTITIES[case["op"]]), case["id"]
        assert all(0.0 <= e < SW.FWD_ATOL / 8 for e in entry.values()), case["id"]
        if case["fn"] in AC.PIECEWISE:
            assert entry["out:dy@kink"] < 1e-7, case["id"]
    assert set(bounds["operators"]) == {"act", "unary"}
    for op, qs in bounds["operators"].items():
        assert set(qs) == set(AC.QUANTITIES[op])
        for q, v in qs.items():
            assert 0.0 < v["median"] <= v["worst"] < SW.FWD_ATOL / 8 and v["n"] == (14 if op == "act" else 7), (op, q, v)


# ------------------------------------------------------------------------------------------------ `check` passes and bites
@pytest.mark.parametrize("case", AC.ALL_CASES, ids=SW.ids(AC.ALL_CASES))
def test_check_passes_the_float32_reference(case, bounds):
    _run_check(case, lambda case, inp, r32: r32, bounds)


@pytest.mark.parametrize("case", AC.ALL_CASES, ids=SW.ids(AC.ALL_CASES))
def test_check_passes_the_float32_restatement_of_the_kernel_formulas(case, bounds):
    _run_check(case, lambda case, inp, r32: AC.split(case, inp, *restate(case, inp["g"])), bounds)


FAULTS = [("act-hard_swish", "hard_swish_le_at_3", "dy@kink"), ("act-relu6", "relu6_grad_1_at_6", "dy@kink"), ("act-relu", "relu_grad_1_at_0", "dy@kink"),
          ("act-selu", "selu_alpha_6th_digit", "@core"), ("act-mish", "mish_no_threshold", "non-finite"), ("unary-softplus_t20", "mish_no_threshold", "non-finite"),
          ("act-tanh", "tanh_exp_2^-16", "y@core"), ("unary-tanh_hw", "tanh_exp_2^-16", "y@core")]


@pytest.mark.parametrize("cid,fault,where", FAULTS, ids=[f"{c}-{f}" for c, f, _ in FAULTS])
def test_check_refuses_the_restatement_with_a_planted_fault(cid, fault, where, bounds):
    """one defect at a time in the restatement that passes above.  The missing threshold of softplus does not change a finite value in
    fp32 (log1p(e^x) rounds to x beyond 20); it shows where e^x overflows: softplus itself is inf there, and a derivative taken through
    it is inf / inf."""
    case = AC.BY_ID[cid]
    with pytest.raises(AssertionError, match=where):
        _run_check(case, lambda case, inp, r32: AC.split(case, inp, *restate(case, inp["g"], fault)), bounds)
