"""CPU tests of the optimizer sweep's own instruments (no GPU): the restatement of tests/optim_reference.py against torch.optim.AdamW with
torch's OneCycleLR and clip_grad_value_ in float64, the torch-ops CPU branch of FusedAdamW.update against the restatement under the rule
the GPU run is held to, the case table of tests/optim_cases.py, and that `check` separates the three mistakes the sweep is there for
(restated on the CPU) from a correct update by orders of magnitude."""
import math
import warnings

import pytest
import torch

import operator_sweep as SW
import optim_cases as OC
import optim_reference as R

CASE_IDS = [c["id"] for c in OC.ALL_CASES]
bounds = SW.bounds_fixture("optim")


def _torch_adamw(case, inp):
    """torch.optim.AdamW on a float64 parameter, the schedule as sast_amd.dist.OneCycleLR documents it (torch's final_div_factor is
    final_div_factor / div_factor), the gradient scaled by hand and clipped by clip_grad_value_ -> (p, m, v) after the first and last step"""
    p = torch.nn.Parameter(inp["p0"].double().clone())
    opt = torch.optim.AdamW([p], lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"])
    sched = None
    if case["schedule"] is not None:
        s = case["schedule"]
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=s["max_lr"], total_steps=s["total_steps"], pct_start=s["pct_start"], anneal_strategy="linear",
                                                    cycle_momentum=False, div_factor=25.0, final_div_factor=10000.0 / 25.0)
    if case["t0"]:          # a resumed run: the step count of the optimizer state and of the scheduler, moments at zero
        opt.state[p] = {"step": torch.tensor(float(case["t0"])), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        sched.last_epoch = case["t0"] - 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)       # (a scheduler step before the first optimizer step: intended here)
            sched.step()
    snaps = []
    for g in inp["grads"]:
        p.grad = g.double() * case["grad_scale"]
        if case["clip"] > 0:
            torch.nn.utils.clip_grad_value_([p], case["clip"])
        opt.step()
        if sched is not None:
            sched.step()
        st = opt.state[p]
        snaps.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return snaps[0], snaps[-1]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_is_torch_adamw_in_float64(cid):
    case = OC.BY_ID[cid]
    inp = OC.make_inputs(case)
    OC.check_conditions(case, inp)
    ref = OC.reference(case, inp, torch.float64)
    want = OC.quantities(inp["p0"], *_torch_adamw(case, inp))
    assert sorted(ref) == sorted(want) == sorted(OC.QUANTITIES)
    for q in OC.QUANTITIES:
        rel = SW.measure(q, ref[q], want[q])[0]
        assert rel <= 1e-12, (cid, q, rel)


@pytest.mark.parametrize("kw", [dict(max_lr=1e-3, total_steps=12, pct_start=0.25), dict(max_lr=1e-3, total_steps=12, pct_start=0.005),
                                dict(max_lr=2e-4, total_steps=2000, pct_start=0.005), dict(max_lr=3e-4, total_steps=50, pct_start=0.3)])
def test_schedule_restatement_is_torch_onecycle_and_the_library_closed_form(kw):
    from sast_amd.dist import OneCycleLR
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, anneal_strategy="linear", cycle_momentum=False, div_factor=25.0, final_div_factor=400.0, **kw)
    mine = OneCycleLR(**kw)
    for step in range(kw["total_steps"]):
        want = opt.param_groups[0]["lr"]
        assert abs(R.onecycle_lr(step, **kw) - want) <= 1e-15 * kw["max_lr"] and abs(mine.lr_at(step) - want) <= 1e-15 * kw["max_lr"], step
        opt.step()
        if step + 1 < kw["total_steps"]:
            sched.step()


@pytest.mark.parametrize("cid", CASE_IDS)
def test_cpu_branch_of_fused_adamw_meets_the_rule_of_the_gpu_run(cid, bounds):
    case = OC.BY_ID[cid]
    inp = OC.make_inputs(case)
    got, lr_step = OC.run_fused(case, inp, torch.device("cpu"))
    SW.check(OC, case, got, OC.reference(case, inp, torch.float64), bounds)
    assert float(lr_step[1]) == case["t0"] + case["steps"]


@pytest.mark.parametrize("name", OC.NONFINITE_NAMES)
def test_cpu_branch_of_fused_adamw_carries_a_nonfinite_gradient_into_the_parameter(name, bounds):
    """the rule of the GPU run's non-finite test on the torch-ops branch, and on torch.optim.AdamW with clip_grad_value_ (clamp_ keeps NaN)"""
    case = next(c for c in OC.ALL_CASES if c["name"] == name)
    inp, where = OC.nonfinite_gradients(case, OC.make_inputs(case))
    assert {v != v or v for v in where.values()} == {True, math.inf, -math.inf} and {1, 2, 3, 257, case["n"] - 1} <= set(where)
    ref = OC.reference(case, inp, torch.float64)
    got, _lr_step = OC.run_fused(case, inp, torch.device("cpu"))
    OC.check_nonfinite(case, got, ref, where, bounds)
    want = OC.quantities(inp["p0"], *_torch_adamw(case, inp))
    for q in OC.QUANTITIES:
        assert torch.equal(torch.isfinite(want[q]), torch.isfinite(ref[q])), q       # (torch's lerp_ turns an infinite moment into NaN a step later)
    swallowed = {q: t.clone() for q, t in got.items()}      # what a clip that drops NaN leaves behind: refused
    for q in ("rel:dp", "rel:m", "rel:v"):
        swallowed[q][list(where)] = 0.0
    with pytest.raises(AssertionError, match="non-finite at"):
        OC.check_nonfinite(case, swallowed, ref, where, bounds)


def test_case_table_covers_what_the_sweep_is_about():
    cs = OC.ALL_CASES
    assert {c["n"] for c in cs} == {4, 1020, 1028, 3076} and all(c["op"] == "adamw" for c in cs)
    assert [c["name"] for c in cs] == ["plain", "wd", "clipscale", "eps1e-3", "betas", "onecycle", "onecycle-nophase1", "onecycle-late"]
    assert sum(c["schedule"] is not None for c in cs) == 3 and sum(c["clip"] > 0 and c["grad_scale"] != 1 for c in cs) == 1
    assert any(c["wd"] > 0 for c in cs) and any(c["eps"] == 1e-3 for c in cs) and any(c["betas"] != (0.9, 0.999) for c in cs)
    assert not any("out:" in q for q in OC.QUANTITIES)


def test_bounds_hold_every_compared_quantity_and_stay_inside_the_project_bar(bounds):
    assert set(bounds["operators"]) == {"adamw"} and set(bounds["operators"]["adamw"]) == set(OC.QUANTITIES)
    for case in OC.ALL_CASES:
        entry = bounds["cases"][case["id"]]
        assert set(entry) == set(OC.QUANTITIES)
        for q, e in entry.items():
            assert 0.0 < e < SW.project_bar(q) / 2, (case["id"], q, e)
    for q, v in bounds["operators"]["adamw"].items():
        assert v["n"] == len(OC.ALL_CASES) and v["median"] < 1e-5, (q, v)


# ------------------------------------------------------------------------------------------------ `check` separates the mistakes
def _mutant(case, inp, what):
    """the float32 restatement with one mistake of the kernel restated"""
    h = OC._hyper(case)
    b1, b2 = h["betas"]

    def run(grads):
        p = inp["p0"].clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for i, g in enumerate(grads):
            t = h["t0"] + i + 1
            sn = t if what == "step-off-by-one" else t - 1
            lr = R.onecycle_lr(sn, **h["schedule"]) if h["schedule"] is not None else h["lr"]
            if what == "clip-before-scale":
                g = g.clamp(-h["clip"], h["clip"]) * h["grad_scale"]
            else:
                g = (g * h["grad_scale"]).clamp(-h["clip"], h["clip"]) if h["clip"] > 0 else g * h["grad_scale"]
            p = p * (1 - lr * h["wd"])
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            bc2 = 1 - b2 ** t
            denom = (v / bc2 + h["eps"]).sqrt() if what == "eps-inside-the-root" else v.sqrt() / math.sqrt(bc2) + h["eps"]
            p = p - (lr / (1 - b1 ** t)) * (m / denom)
        return p, m, v
    return OC.quantities(inp["p0"], run(inp["grads"][:1]), run(inp["grads"]))


@pytest.mark.parametrize("what,name", [(None, "onecycle"), ("step-off-by-one", "onecycle"), ("step-off-by-one", "onecycle-nophase1"),
                                       ("clip-before-scale", "clipscale"), ("eps-inside-the-root", "eps1e-3"), ("eps-inside-the-root", "plain")])
def test_check_refuses_the_mistakes_the_sweep_is_there_for(what, name, bounds):
    case = next(c for c in OC.ALL_CASES if c["name"] == name)
    inp = OC.make_inputs(case)
    ref, got = OC.reference(case, inp, torch.float64), _mutant(case, inp, what)
    if what is None:
        SW.check(OC, case, got, ref, bounds)
        return
    with pytest.raises(AssertionError, match="rel:dp"):
        SW.check(OC, case, got, ref, bounds)
    assert SW.measure("rel:dp", got["rel:dp"], ref["rel:dp"])[0] > 1e-2       # four orders of magnitude over the float32 noise
