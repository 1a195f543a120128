"""The case table of the optimizer sweep (tests/test_optim_operators.py: the fused AdamW kernel of csrc/k_conv.hip behind sast_adamw and
sast_adamw_onecycle), the inputs of every case and its CPU reference.  The fourth suite of tests/operator_sweep.py ("optim"), shared by
the GPU test, the bounds generator and tests/test_optim_reference.py.  CPU only: importing this module does not import the library
(`run_fused`, the one driver of sast_amd.dist.FusedAdamW for the CPU and the GPU test, imports it when called).

Operator "adamw".  Quantities, every one relative to the reference tensor's max-norm (no name carries "out:"):
  rel:dp   the cumulative update p_n - p_0 (p itself would hide an lr-sized error behind the parameter's size)
  rel:m, rel:v   the moments
each after the last step, and with the suffix "@1" after the first.

Inputs: p0 = randn / 64 (with |p| of order 1 the float32 rounding of p alone would cost 1e-4 of an lr-sized update; here the float32
restatement stays within a few 1e-6 of float64); one gradient per step, scale * randn with every 7th element exactly 0 (denom reduces to
eps there, m and v stay 0).  Sizes n = 4 (one float4), 1020 (a partial block of 256 float4), 1028 (one float4 into a second block) and
3076 (three blocks plus one) are spread over the cases.

  plain              lr 1e-3, 5 steps
  wd                 weight_decay 0.5
  clipscale          gradients of order 8, grad_scale 1 / 8, clip 1.0: about a third of the elements clip, and only if the scale comes first
  eps1e-3            the eps of the TrainStep tests, gradients of order 1e-3: eps is a third of denom, inside the root it would be 30 x that
  betas              (0.8, 0.99)
  onecycle           max_lr 1e-3, 12 steps of 12, pct_start 0.25: both phases, the peak and the final min_lr
  onecycle-nophase1  the reference's pct_start 0.005 at 12 steps: end1 < 0, the second branch runs from the first step
  onecycle-late      max_lr 2e-4 over 400 000 steps, the step counter preset to 399 990, 8 steps; p0 = 0 (the lr is 2e-8 there: any other
                     p0 would swallow the update); both bias corrections are 1 in float32
"""
import sys

import torch

import operator_sweep as SW
import optim_reference as R


def _case(name, n, steps, gscale=1.0, gsize=1e-2, **opt):
    c = dict(id=f"adamw-{name}-n{n}", name=name, op="adamw", n=n, steps=steps, gsize=gsize, lr=1e-3, schedule=None, betas=(0.9, 0.999), eps=1e-8, wd=0.0,
             grad_scale=gscale, clip=0.0, t0=0, zero_p0=False, env={})
    c.update(opt)
    return c


ALL_CASES = [
    _case("plain", 1028, 5),
    _case("wd", 3076, 5, wd=0.5),
    _case("clipscale", 1020, 5, gscale=0.125, gsize=8.0, clip=1.0),
    _case("eps1e-3", 1028, 5, gsize=1e-3, eps=1e-3),
    _case("betas", 4, 5, betas=(0.8, 0.99)),
    _case("onecycle", 3076, 12, schedule=dict(max_lr=1e-3, total_steps=12, pct_start=0.25)),
    _case("onecycle-nophase1", 1020, 12, schedule=dict(max_lr=1e-3, total_steps=12, pct_start=0.005)),
    _case("onecycle-late", 1028, 8, schedule=dict(max_lr=2e-4, total_steps=400000, pct_start=0.005), t0=399990, zero_p0=True),
]
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"
QUANTITIES = ("rel:dp", "rel:m", "rel:v", "rel:dp@1", "rel:m@1", "rel:v@1")


def bounds_id(case):
    return case["id"]


def pool_key(quantity):
    return quantity


def make_inputs(case):
    g = SW.gen(case["id"])
    n = case["n"]
    p0 = torch.zeros(n) if case["zero_p0"] else torch.randn(n, generator=g) / 64
    grads = []
    for _ in range(case["steps"]):
        gr = case["gsize"] * torch.randn(n, generator=g)
        gr[::7] = 0.0
        grads.append(gr)
    return {"p0": p0, "grads": grads}


def check_conditions(case, inp):
    n, sched = case["n"], case["schedule"]
    assert n % 4 == 0 and tuple(inp["p0"].shape) == (n,) and len(inp["grads"]) == case["steps"]
    assert all(float(g[::7].abs().max()) == 0.0 and float(g.abs().max()) > 0.0 for g in inp["grads"])
    assert (float(inp["p0"].abs().max()) == 0.0) == case["zero_p0"] and float(inp["p0"].abs().max()) < 0.1
    if case["clip"] > 0:        # a good share of the elements clips after the scale, and every non-zero one would clip before it
        big = torch.stack(inp["grads"])
        frac = float(((big * case["grad_scale"]).abs() > case["clip"]).float().mean())
        assert 0.2 < frac < 0.4 and float((big.abs() > case["clip"]).float().mean()) > 0.7
    if sched is not None:
        end1 = sched["pct_start"] * sched["total_steps"] - 1
        steps = range(case["t0"], case["t0"] + case["steps"])
        lrs = [R.onecycle_lr(s, **sched) for s in steps]
        if case["name"] == "onecycle":
            assert end1 == 2.0 and any(s < end1 for s in steps) and any(s > end1 for s in steps)
            assert abs(max(lrs) - sched["max_lr"]) < 1e-18 and lrs[2] == max(lrs) and abs(lrs[-1] - sched["max_lr"] / 1e4) < 1e-18 and lrs[0] == sched["max_lr"] / 25
        elif case["name"] == "onecycle-nophase1":
            assert end1 < 0 and all(a > b for a, b in zip(lrs, lrs[1:])) and lrs[0] < sched["max_lr"]
        else:
            assert case["t0"] + case["steps"] < sched["total_steps"] and max(lrs) < 1e-4 * sched["max_lr"] * 2
            assert float(torch.tensor(1 - 0.9 ** case["t0"], dtype=torch.float32)) == 1.0 == float(torch.tensor(1 - 0.999 ** case["t0"], dtype=torch.float32))


def _hyper(case):
    return dict(lr=case["lr"], schedule=case["schedule"], betas=case["betas"], eps=case["eps"], wd=case["wd"], grad_scale=case["grad_scale"],
                clip=case["clip"], t0=case["t0"])


def quantities(p0, after_first, after_last):
    out = {}
    for tag, (p, m, v) in (("@1", after_first), ("", after_last)):
        out["rel:dp" + tag] = p.detach().double().cpu() - p0.double()
        out["rel:m" + tag], out["rel:v" + tag] = m.detach().cpu().clone(), v.detach().cpu().clone()
    return out


def reference(case, inp, dtype):
    h = _hyper(case)
    return quantities(inp["p0"], R.adamw(inp["p0"], inp["grads"][:1], dtype, **h), R.adamw(inp["p0"], inp["grads"], dtype, **h))


class Holder(torch.nn.Module):
    def __init__(self, p0):
        super().__init__()
        self.w = torch.nn.Parameter(p0.clone())


def make_optimizer(case, p0, device):
    """(FlatParams over one parameter holding p0, FusedAdamW as the case configures it)"""
    from sast_amd.dist import FlatParams, FusedAdamW, OneCycleLR
    fp = FlatParams([Holder(p0).to(device)])
    assert fp.numel == case["n"]
    sched = OneCycleLR(**case["schedule"]) if case["schedule"] is not None else None
    opt = FusedAdamW(fp, lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"], clip_value=case["clip"], schedule=sched)
    opt.lr_step[1] = float(case["t0"])
    return fp, opt


def run_fused(case, inp, device):
    """the case through FusedAdamW on `device` (cuda: the kernel; cpu: its torch-ops branch) -> the quantities, and the final lr_step"""
    fp, opt = make_optimizer(case, inp["p0"], device)
    first = None
    for g in inp["grads"]:
        fp.grad.copy_(g)
        opt.step(case["grad_scale"])
        if first is None:
            first = (fp.flat.clone(), opt.m.clone(), opt.v.clone())
    return quantities(inp["p0"], first, (fp.flat, opt.m, opt.v)), opt.lr_step.detach().cpu()


# ------------------------------------------------------------------------------------------------ non-finite gradients
# torch clips by value with clamp_, which keeps NaN; IEEE fminf / fmaxf return the other operand and would turn a NaN gradient into an
# update of -clip that leaves m and v finite.  Three cases (no clip, clip after the scale, the schedule on the device) with NaN, +Inf and
# -Inf written over a few elements of the SECOND gradient: the first float4 (all three in one vector), the first float4 of the second
# block and the last float4 -- which at these sizes is, or lies in, the partial last block.  None is a multiple of 7 (the exact zeros).
NONFINITE_NAMES = ("plain", "clipscale", "onecycle")
NONFINITE_STEP = 1          # index into inp["grads"]: optimizer step 2


def nonfinite_gradients(case, inp):
    """(the inputs with the poisoned second gradient, {index: the value written there})"""
    n, vals = case["n"], (float("nan"), float("inf"), -float("inf"))
    last = [i for i in range(n - 4, n) if i % 7][-3:]
    where = dict(zip([1, 2, 3] + last, vals + vals))
    where[257] = vals[0]
    assert len(last) == 3 and all(i % 7 and 0 < i < n for i in where) and n - 4 >= (n - 1) // 1024 * 1024 and (n // 4) % 256
    grads = [g.clone() for g in inp["grads"]]
    for i, val in where.items():
        grads[NONFINITE_STEP][i] = val
    return dict(inp, grads=grads), where


def check_nonfinite(case, got, ref, where, bounds):
    """the non-finite mask of every quantity equals the float64 reference's (empty after the first step; after the last every poisoned
    element, but the +-Inf ones of a clipping case, which clip to +-clip); every other element passes the case's `check`"""
    hit = torch.zeros(case["n"], dtype=torch.bool)
    hit[[i for i, val in where.items() if not (case["clip"] > 0 and val == val)]] = True
    assert bool(hit.any())
    for q in QUANTITIES:
        bad = ~torch.isfinite(ref[q])
        assert torch.equal(bad, hit if "@" not in q else torch.zeros_like(hit)), (case["id"], q, bad.nonzero().view(-1).tolist())
        mine = ~torch.isfinite(got[q])
        assert torch.equal(mine, bad), f"{case['id']}: {q} is non-finite at {mine.nonzero().view(-1).tolist()}, the reference at {bad.nonzero().view(-1).tolist()}"
        if "@" not in q and "rel:m" in q:       # where a value is defined it is the reference's: NaN stays NaN, an infinite moment keeps its sign
            inf = bad & ~torch.isnan(ref[q])
            assert torch.equal(torch.isnan(got[q]), torch.isnan(ref[q])) and torch.equal(got[q][inf].double(), ref[q][inf].double())
    keep = ~hit
    SW.check(sys.modules[__name__], case, {q: got[q][keep] for q in QUANTITIES}, {q: ref[q][keep] for q in QUANTITIES}, bounds)


BOUNDS_CASES = ALL_CASES
float_quantities = sorted
DISCRETE = ()
