"""The case table of the elementwise sweep (tests/test_act_operators.py: the 14-way gate activation `glu_act` / `glu_act_grad` of the
GLU-MLP epilogues and the fast-math helpers of csrc/common.cuh, reached on their own through sast_test_glu_act / sast_test_unary of the
tools library), the points every case is evaluated on and its CPU reference.  The sixth suite of tests/operator_sweep.py ("act"), shared
by the GPU test, the bounds generator and tests/test_act_reference.py.  CPU only: nothing here imports the library.

A case is one function: an activation code with its hand-written derivative (operator "act": y and dy) or one helper (operator "unary":
y only).  prelu runs with slope 0.3.

Points (`points()`; exact fp32 values, no random generator, the same for every case; rsqrt_hw takes the positive normal ones):
  * the grid k / 1024 over [-24, 24]: it holds every kink of the table (0, +-2, +-3, 6, 20) exactly;
  * every kink +- 1 .. 4 ulps (around 0: the four smallest subnormals of either sign);
  * +-2^e (1 + j / 8) for e in [-126, 6], j < 8;
  * +-0, +-FLT_MIN, the smallest subnormal of either sign, +-88, +-89, +-100 (e^88 is finite in fp32, e^89 is not).

Reference: torch on the float64 image of the points, derivatives from autograd (hard_mish: the oracle's formula), so that a point on a
kink gets torch's convention.  Quantities, split so that rounding at large |g| cannot hide an error near 0:
  out:y@core, out:dy@core   |g| <= 4
  out:y@tail, out:dy@tail   |g| > 4, both sides divided in float64 by max(1, |g|)
  out:dy@kink               the points on a kink and their ulp neighbours (float32, undivided); bit-equal to the float32 reference
                            for the piecewise-linear activations (PIECEWISE), whose derivatives there are exact in fp32
rsqrt_hw is the one function whose value is not O(max(1, |g|)): its two quantities are divided by max(1, g^-1/2) instead -- a function
of the point alone, like the other divisor -- which makes them relative where rsqrt is large.  Subnormal arguments are left out for it:
v_rsq_f32 flushes them by specification, and every call site passes a variance plus an eps of 1e-5 or more.
"""
import torch
import torch.nn.functional as F

from oracle import sast_oracle as O

# csrc/common.cuh: the codes of glu_act (sast_amd.functional.GLU_ACTIVATIONS holds the same, with aliases)
ACT_CODES = {"gelu": 0, "relu": 1, "silu": 2, "sigmoid": 3, "tanh": 4, "mish": 5, "relu6": 6, "leaky_relu": 7, "elu": 8, "selu": 9,
             "hard_sigmoid": 10, "hard_swish": 11, "hard_mish": 12, "prelu": 13}
UNARY_CODES = {"sigmoid_hw": 0, "tanh_hw": 1, "gelu_erf": 2, "gelu_erf_grad": 3, "softplus_t20": 4, "rsqrt_hw": 5, "silu": 6}
PRELU_SLOPE = 0.3
# where each activation's derivative jumps or its formula changes branch
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0), "leaky_relu": (0.0,), "prelu": (0.0,), "elu": (0.0,), "selu": (0.0,), "hard_sigmoid": (-3.0, 3.0),
         "hard_swish": (-3.0, 3.0), "hard_mish": (-2.0, 0.0), "mish": (20.0,)}
ALL_KINKS = (-3.0, -2.0, 0.0, 2.0, 3.0, 6.0, 20.0)
PIECEWISE = ("relu", "relu6", "leaky_relu", "hard_sigmoid", "hard_swish", "hard_mish", "prelu")
CORE = 4.0
FLT_MIN, DENORM_MIN = 2.0 ** -126, 2.0 ** -149


def _act(name):
    return dict(id=f"act-{name}", op="act", fn=name, code=ACT_CODES[name], slope=PRELU_SLOPE if name == "prelu" else 0.0, env={})


def _unary(name):
    return dict(id=f"unary-{name}", op="unary", fn=name, code=UNARY_CODES[name], slope=0.0, env={})


ACT_CASES = [_act(n) for n in ACT_CODES]
UNARY_CASES = [_unary(n) for n in UNARY_CODES]
ALL_CASES = ACT_CASES + UNARY_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"
QUANTITIES = {"act": ("out:dy@core", "out:dy@kink", "out:dy@tail", "out:y@core", "out:y@tail"), "unary": ("out:y@core", "out:y@tail")}


def bounds_id(case):
    return case["id"]


def pool_key(quantity):
    return quantity


# ------------------------------------------------------------------------------------------------ the points
def kink_points():
    """every kink and its four fp32 neighbours on either side, ascending per kink"""
    out = []
    for k in ALL_KINKS:
        c = torch.tensor(k, dtype=torch.float32)
        lo, hi = [c], [c]
        for _ in range(4):
            lo.append(torch.nextafter(lo[-1], torch.tensor(-float("inf"))))
            hi.append(torch.nextafter(hi[-1], torch.tensor(float("inf"))))
        out += lo[:0:-1] + [c] + hi[1:]
    return torch.stack(out)


_POINTS = None


def points():
    """(the points, float32; the mask of the kink neighbourhoods)"""
    global _POINTS
    if _POINTS is None:
        grid = torch.arange(-24 * 1024, 24 * 1024 + 1, dtype=torch.float64) / 1024
        mant = 1 + torch.arange(8, dtype=torch.float64) / 8
        octaves = (2.0 ** torch.arange(-126, 7, dtype=torch.float64))[:, None] * mant[None, :]
        special = torch.tensor([0.0, -0.0, FLT_MIN, -FLT_MIN, DENORM_MIN, -DENORM_MIN, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0], dtype=torch.float64)
        kink = kink_points()
        rest = torch.cat([grid, octaves.reshape(-1), -octaves.reshape(-1), special])
        assert torch.equal(rest.float().double(), rest), "a point is not an exact fp32 value"
        g = torch.cat([kink, rest.float()])
        is_kink = torch.zeros(g.numel(), dtype=torch.bool)
        is_kink[:kink.numel()] = True
        _POINTS = (g, is_kink)
    return _POINTS


def make_inputs(case):
    g, is_kink = points()
    if case["fn"] == "rsqrt_hw":
        keep = g >= FLT_MIN
        g, is_kink = g[keep], is_kink[keep]
    return {"g": g.clone(), "kink": is_kink.clone().to(torch.uint8)}


def check_conditions(case, inp):
    g = inp["g"].double()
    assert inp["g"].dtype == torch.float32 and bool(torch.isfinite(g).all())
    have = set(g.tolist())
    assert {88.0, 89.0, 100.0, FLT_MIN, 24.0, 4.0, 2.0, 3.0, 6.0, 20.0} <= have
    if case["fn"] == "rsqrt_hw":
        assert float(g.min()) == FLT_MIN
    else:
        assert set(ALL_KINKS) <= have and {-88.0, -89.0, -100.0, -24.0, DENORM_MIN, -DENORM_MIN, -FLT_MIN} <= have and bool((inp["g"] == 0).sum() >= 2)
        assert int(inp["kink"].sum()) == 9 * len(ALL_KINKS)
        for k in ALL_KINKS:         # four distinct neighbours on either side of every kink
            near = inp["kink"].bool() & ((g - k).abs() <= 1e-5)
            assert int((near & (g > k)).sum()) == 4 == int((near & (g < k)).sum()) and int((near & (g == k)).sum()) == 1, k
    assert (2e4 if case["fn"] == "rsqrt_hw" else 5e4) < g.numel() < 7e4


# ------------------------------------------------------------------------------------------------ reference evaluation
def _grad_of(f):
    def df(x):
        x = x.detach().clone().requires_grad_(True)
        return torch.autograd.grad(f(x).sum(), x)[0]
    return df


UNARY_REFS = {"sigmoid_hw": torch.sigmoid, "tanh_hw": torch.tanh, "gelu_erf": F.gelu, "gelu_erf_grad": _grad_of(F.gelu), "softplus_t20": F.softplus,
              "rsqrt_hw": torch.rsqrt, "silu": F.silu}


def evaluate_reference(case, g):
    """(y, dy or None) of the case's function in the dtype of `g`"""
    if case["op"] == "unary":
        return UNARY_REFS[case["fn"]](g).detach(), None
    x = g.detach().clone().requires_grad_(True)
    if case["fn"] == "prelu":
        y = F.prelu(x, torch.tensor([case["slope"]], dtype=torch.float32).to(g.dtype))
    else:
        y = O.GLU_ACTS[case["fn"]](x)
    return y.detach(), torch.autograd.grad(y.sum(), x)[0]


def split(case, inp, y, dy):
    """the suite's quantities of one evaluation (y, dy: one value per point, any float dtype)"""
    g = inp["g"].double()
    core, kink = g.abs() <= CORE, inp["kink"].bool()
    div = torch.clamp(g.rsqrt(), min=1.0) if case["fn"] == "rsqrt_hw" else torch.where(core, torch.ones_like(g), g.abs())
    out = {}
    for name, t in (("y", y), ("dy", dy)):
        if t is None:
            continue
        t = t.detach().cpu()
        assert t.shape == g.shape
        out[f"out:{name}@core"] = (t.double() / div)[core]
        out[f"out:{name}@tail"] = (t.double() / div)[~core]
    if dy is not None:
        out["out:dy@kink"] = dy.detach().cpu()[kink].clone()
    return out


def reference(case, inp, dtype):
    y, dy = evaluate_reference(case, inp["g"].to(dtype))
    return split(case, inp, y, dy)


def bit_equal(case, r32):
    """the `bit_equal` argument of `check` for this case, from its float32 reference"""
    return {"out:dy@kink": r32["out:dy@kink"]} if case["fn"] in PIECEWISE and case["op"] == "act" else {}


BOUNDS_CASES = list(ALL_CASES)
float_quantities = sorted
DISCRETE = ()
