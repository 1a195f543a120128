"""The fused AdamW kernel (csrc/k_conv.hip: adamw_kernel behind sast_adamw and sast_adamw_onecycle) through sast_amd.dist.FusedAdamW on a
FlatParams, against the float64 restatement of tests/optim_reference.py on the cases of tests/optim_cases.py: the fourth suite of
tests/operator_sweep.py.

Compared, after the first and after the last step: the cumulative update p_n - p_0 and both moments, each relative to the reference
tensor's max-norm, under the two bars of the other sweeps -- the project's GRAD_RTOL = 3e-4 and FACTOR x max(e32 of the case, median e32 of
the operator), where e32 is the error of the float32 CPU restatement against float64 (tests/golden/optim_operator_bounds.json: never a
figure the kernel produced).  An off-by-one in the schedule's step, the clip in front of grad_scale or eps inside the square root move
the update by 16 .. 90 %, four to five orders of magnitude above these bounds (tests/test_optim_reference.py shows `check` refusing each).

Beyond the sweep: per-bucket updates against one whole-buffer update and a graph-captured step against eager steps, both bit for bit,
and the argument errors.
"""
import pytest
import torch

import operator_sweep as SW
import optim_cases as OC
from operator_sweep import SAST_EINVAL, check, dev, ids, restore_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

bounds = SW.bounds_fixture("optim")


@pytest.mark.parametrize("case", OC.ALL_CASES, ids=ids(OC.ALL_CASES))
def test_fused_adamw(case, dev, bounds):
    """no clip / clip after grad_scale, weight decay, the eps of the training tests, other betas, the OneCycleLR branch on the device in
    both phases, from the first step without a first phase and near the end of a long run; n = one float4 .. three blocks plus one"""
    inp = OC.make_inputs(case)
    OC.check_conditions(case, inp)
    got, lr_step = OC.run_fused(case, inp, dev)
    check(OC, case, got, OC.reference(case, inp, torch.float64), bounds)
    assert float(lr_step[1]) == case["t0"] + case["steps"]
    if case["schedule"] is None:
        assert float(lr_step[0]) == float(torch.tensor(case["lr"], dtype=torch.float32))
    zero = got["rel:m"][::7]
    assert float(zero.abs().max()) == 0.0 and float(got["rel:v"][::7].abs().max()) == 0.0       # a zero gradient leaves the moments at zero


NONFINITE_CASES = [c for c in OC.ALL_CASES if c["name"] in OC.NONFINITE_NAMES]


@pytest.mark.parametrize("case", NONFINITE_CASES, ids=ids(NONFINITE_CASES))
def test_fused_adamw_carries_a_nonfinite_gradient_into_the_parameter(case, dev, bounds):
    """NaN, +Inf and -Inf in the second gradient (first float4, second block, last float4): the non-finite elements of the update and of
    both moments are the float64 reference's after the first and the last step -- a clip by fminf / fmaxf would turn the NaN into an
    update of -clip and leave m and v finite -- and every other element stays inside the case's bounds"""
    inp, where = OC.nonfinite_gradients(case, OC.make_inputs(case))
    got, lr_step = OC.run_fused(case, inp, dev)
    OC.check_nonfinite(case, got, OC.reference(case, inp, torch.float64), where, bounds)
    assert float(lr_step[1]) == case["t0"] + case["steps"]


def _three_modules(dev):
    torch.manual_seed(3)
    return [torch.nn.Linear(5, 3).to(dev), torch.nn.Linear(7, 2).to(dev), torch.nn.Linear(3, 3, bias=False).to(dev)]


def test_bucket_updates_equal_one_whole_buffer_update(dev):
    """three buckets updated one by one (begin_step, then update(bucket=i)) == one update of the whole buffer, bit for bit; every
    parameter size is no multiple of 4, so every bucket has padding slots"""
    from sast_amd.dist import FlatParams, FusedAdamW, OneCycleLR
    mods, twins = _three_modules(dev), _three_modules(dev)
    fp, fq = FlatParams(mods, buckets=[[m] for m in mods]), FlatParams(twins)
    assert all(p.numel() % 4 for p in fp.params) and fp.numel == fq.numel == sum((p.numel() + 3) // 4 * 4 for p in fp.params) > sum(p.numel() for p in fp.params)
    assert len(fp.bucket_ranges) == 3 and all(b > a and a % 4 == 0 and b % 4 == 0 for a, b in fp.bucket_ranges) and fp.bucket_ranges[-1][1] == fp.numel
    assert torch.equal(fp.flat, fq.flat)
    start = fp.flat.clone()
    kw = dict(betas=(0.9, 0.999), eps=1e-3, weight_decay=0.05, clip_value=1.0)
    opt, whole = (FusedAdamW(f, schedule=OneCycleLR(1e-3, total_steps=12, pct_start=0.25), **kw) for f in (fp, fq))
    g = torch.Generator().manual_seed(5)
    for _step in range(4):
        grad = (torch.randn(fp.numel, generator=g) * 2).to(dev)
        fp.grad.copy_(grad)
        fq.grad.copy_(grad)
        opt.begin_step()
        for i in range(3):
            opt.update(0.5, bucket=i)
        whole.step(0.5)
        torch.cuda.synchronize()
        for name, a, b in (("flat", fp.flat, fq.flat), ("m", opt.m, whole.m), ("v", opt.v, whole.v), ("lr_step", opt.lr_step, whole.lr_step)):
            assert torch.equal(a, b), (name, _step)
    assert float(opt.lr_step[1]) == 4.0 and not torch.equal(fp.flat, start)


def test_captured_step_replays_the_schedule(dev):
    """opt.step() (counter add + kernel) captured once and replayed on new gradients == eager steps of a twin, bit for bit, on the
    `onecycle` case; the counter advanced with the replays"""
    case = next(c for c in OC.ALL_CASES if c["name"] == "onecycle")
    inp = OC.make_inputs(case)
    grads = [g.to(dev) for g in inp["grads"][:5]]
    fp, opt = OC.make_optimizer(case, inp["p0"], dev)
    fq, twin = OC.make_optimizer(case, inp["p0"], dev)
    fp.grad.copy_(grads[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.step(case["grad_scale"])                     # the warm-up is a real step: put the state back
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert float(opt.lr_step[1]) == 1.0 and not torch.equal(fp.flat, fq.flat)
    fp.flat.copy_(fq.flat)
    opt.m.zero_()
    opt.v.zero_()
    opt.lr_step[1] = 0.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step(case["grad_scale"])
    for k, grad in enumerate(grads):
        fp.grad.copy_(grad)
        g.replay()
        fq.grad.copy_(grad)
        twin.step(case["grad_scale"])
        torch.cuda.synchronize()
        for name, a, b in (("flat", fp.flat, fq.flat), ("m", opt.m, twin.m), ("v", opt.v, twin.v), ("lr_step", opt.lr_step, twin.lr_step)):
            assert torch.equal(a, b), (name, k)
    assert float(opt.lr_step[1]) == 5.0
    assert not torch.equal(fp.flat.cpu(), inp["p0"])


def test_adamw_refuses_bad_arguments(dev):
    from sast_amd import _lib as L, functional as SF
    lib = L.lib()
    p, g, m, v = (torch.full((8,), 0.5, device=dev) for _ in range(4))
    lr_step = torch.tensor([1e-3, 1.0], device=dev)
    ptrs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr())
    tail = (0.9, 0.999, 1e-8, 0.0, 1.0, 0.0)
    for n in (6, 7, 1):
        assert lib.sast_adamw(*ptrs, n, lr_step.data_ptr(), *tail, SF._stream()) == SAST_EINVAL
        assert lib.sast_adamw_onecycle(*ptrs, n, lr_step.data_ptr(), *tail, 4e-5, 1e-3, 1e-7, 2.0, 11.0, SF._stream()) == SAST_EINVAL
    for end1, end2 in ((11.0, 11.0), (11.0, 2.0)):
        assert lib.sast_adamw_onecycle(*ptrs, 8, lr_step.data_ptr(), *tail, 4e-5, 1e-3, 1e-7, end1, end2, SF._stream()) == SAST_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 0.5).all()) for t in (p, g, m, v))           # refused before anything ran
    assert lib.sast_adamw_onecycle(*ptrs, 8, lr_step.data_ptr(), *tail, 4e-5, 1e-3, 1e-7, 2.0, 11.0, SF._stream()) == 0
    torch.cuda.synchronize()
    assert not bool((p == 0.5).any())
