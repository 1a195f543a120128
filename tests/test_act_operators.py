"""The elementwise arithmetic of csrc/common.cuh on its own (sast_test_glu_act / sast_test_unary of the tools library: `glu_act` and
`glu_act_grad` under every activation code, and sigmoid_hw, tanh_hw, gelu_erf, gelu_erf_grad, softplus_t20, rsqrt_hw and the SiLU of the
conv epilogues) against torch in float64 on the points of tests/act_cases.py: the sixth suite of tests/operator_sweep.py.

About 5 * 10^4 exact fp32 points per function: a grid of 2^-10 over [-24, 24], every kink of every activation with its four fp32
neighbours on either side, every binade from FLT_MIN to 64, subnormals, and both sides of the overflow of e^x.  Compared: y and dy on
|g| <= 4, y / max(1, |g|) and dy / max(1, |g|) beyond, and dy on the kink neighbourhoods -- bit for bit for the piecewise-linear
activations -- under the bars of the other sweeps: FACTOR x max(e32 of the case, median e32 of the operator), where e32 is the error of
torch's float32 CPU evaluation against float64 (tests/golden/act_operator_bounds.json: never a figure the kernels produced).

Memory discipline: the outputs are NaN on the n points (an element the kernel does not write fails the finiteness test of `check`) and
a sentinel on TAIL elements behind them, which must come back bit for bit; the input comes back unchanged.
"""
import ctypes as C

import pytest
import torch

import act_cases as AC
import operator_sweep as SW
from operator_sweep import SAST_EINVAL, check, dev, ids, restore_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

bounds = SW.bounds_fixture("act")
TAIL = 1024
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def tools():
    from sast_amd import _lib as L
    lib = L.tools_lib()
    lib.sast_test_glu_act.restype = C.c_int
    lib.sast_test_glu_act.argtypes = [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_float, C.c_void_p]
    lib.sast_test_unary.restype = C.c_int
    lib.sast_test_unary.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p]
    return lib


def _output(n, dev):
    out = torch.full((n + TAIL,), float("nan"), device=dev)
    out[n:] = SENTINEL
    return out


def run_case(tools, case, inp, dev):
    """(y, dy or None) of the case's function on the device, CPU tensors"""
    from sast_amd import functional as SF
    g, n, st = inp["g"].to(dev), inp["g"].numel(), SF._stream()
    y, dy = _output(n, dev), _output(n, dev)
    if case["op"] == "act":
        rc = tools.sast_test_glu_act(g.data_ptr(), y.data_ptr(), dy.data_ptr(), n, case["code"], case["slope"], st)
    else:
        rc = tools.sast_test_unary(g.data_ptr(), y.data_ptr(), n, case["code"], st)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((y[n:] == SENTINEL).all()) and bool((dy[n:] == SENTINEL).all()), "the kernel wrote behind the last point"
    assert torch.equal(g.cpu().view(torch.int32), inp["g"].view(torch.int32)), "the kernel changed its input"
    if case["op"] == "unary":
        assert bool(torch.isnan(dy[:n]).all())
        return y[:n].cpu(), None
    return y[:n].cpu(), dy[:n].cpu()


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.fixture(scope="module")
def references():
    """{case id: (inputs, float64 reference, float32 reference)}, evaluated once"""
    out = {}
    for case in AC.ALL_CASES:
        inp = AC.make_inputs(case)
        AC.check_conditions(case, inp)
        out[case["id"]] = (inp, AC.reference(case, inp, torch.float64), AC.reference(case, inp, torch.float32))
    return out


def _worst(inp, got, ref, q):
    d = (got[q].double() - ref[q].double()).abs()
    g = inp["g"].double()
    sel = inp["kink"].bool() if q.endswith("@kink") else (g.abs() <= AC.CORE) if q.endswith("@core") else (g.abs() > AC.CORE)
    return float(g[sel][int(d.argmax())])


@pytest.mark.parametrize("case", AC.ALL_CASES, ids=ids(AC.ALL_CASES))
def test_function(case, dev, bounds, tools, references):
    inp, ref, r32 = references[case["id"]]
    got = AC.split(case, inp, *run_case(tools, case, inp, dev))
    for q in sorted(ref):
        print(f"{case['id']:24s} {q:14s} worst point g = {_worst(inp, got, ref, q)!r}")
    check(AC, case, got, ref, bounds, bit_equal=AC.bit_equal(case, r32))


# ------------------------------------------------------------------------------------------------ NaN and the infinities
def test_functions_at_nan_and_the_infinities(dev, bounds, tools):
    """NaN, +Inf and -Inf through all 14 activation codes and the helpers (rsqrt_hw aside: its callers pass a variance plus eps) against
    torch in float64: NaN where torch gives NaN (a clamp written with fminf / fmaxf returns the bound instead), non-finite where torch is
    non-finite, and where torch is finite (a saturated gate, the clamps at an infinity) the same value within the case's `out:y@tail`
    bound.  The derivatives are not compared at these points: torch's own conventions at NaN are not uniform."""
    pts = torch.tensor([float("nan"), float("inf"), -float("inf")])
    misses = []
    for case in AC.ALL_CASES:
        if case["fn"] == "rsqrt_hw":
            continue
        want, _dy = AC.evaluate_reference(case, pts.double())
        y, _dy = run_case(tools, case, {"g": pts}, dev)
        e32, med = bounds["cases"][case["id"]]["out:y@tail"], bounds["operators"][case["op"]]["out:y@tail"]["median"]
        tol = min(SW.project_bar("out:y@tail"), SW.FACTOR * max(e32, med))
        for g, a, b in zip(pts.tolist(), y.tolist(), want.tolist()):
            print(f"{case['id']:24s} g = {g!r:5}  y = {a!r}  torch {b!r}")
            if b != b:
                ok = a != a
            elif abs(b) == float("inf"):
                ok = a == b
            else:
                ok = abs(a - b) <= tol
            if not ok:
                misses.append(f"{case['id']} at {g!r}: {a!r}, torch gives {b!r}")
    assert not misses, "\n  ".join(misses)


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_codes_outside_their_tables(dev, tools):
    from sast_amd import functional as SF
    st, n = SF._stream(), 300
    g = torch.linspace(-3, 3, n, device=dev)
    for act in (-1, 14, 1 << 20):
        y, dy = torch.full((n,), SENTINEL, device=dev), torch.full((n,), SENTINEL, device=dev)
        assert tools.sast_test_glu_act(g.data_ptr(), y.data_ptr(), dy.data_ptr(), n, act, 0.0, st) == SAST_EINVAL, act
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()) and bool((dy == SENTINEL).all()), act
    for fn in (-1, 7, 1 << 20):
        y = torch.full((n,), SENTINEL, device=dev)
        assert tools.sast_test_unary(g.data_ptr(), y.data_ptr(), n, fn, st) == SAST_EINVAL, fn
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), fn
