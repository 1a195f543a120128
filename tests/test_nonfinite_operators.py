"""NaN and Inf through the operators: containment and propagation (include/sast_hip.h, "Non-finite values").

Every finite-input sweep is blind to how a kernel ignores a value: `0 * x` and `select(0, x)` agree on finite data and differ only for
NaN / Inf.  Here part P of an operator's input is poisoned (tests/nonfinite_cases.py: the last sample, one pixel, the rows a selection
does not keep, the masked rows) and the device is run with P := 0 twice (g0, g0'), P := NaN (gN) and P := +Inf (gI) through the runners
of the conv and token sweeps.  The float64 reference says which result elements may depend on P (I: independent, D: dependent, A: the
reference itself multiplies the poison by zero).  Per quantity:
  1. on I (minus A for an "either" recipe) gN and gI are finite,
  2. and equal g0 there: bit for bit where g0 and g0' are bit-equal, else (atomic accumulation order) within the project's bars
     FWD_ATOL / GRAD_RTOL as `operator_sweep.measure` applies them -- no tolerance of this test's own.  For the sums over rows
     (parameter gradients, running statistics: float atomics, split-R jobs) two equal zero-filled runs prove nothing: at 212 kept
     rows nine runs of one input gave d fc2_b the bit patterns 0 0 0 1 0 1 0 0 1 and d proj_b 0 1 2 2 3 1 3 3 3, whatever the fill, so
     g0 == g0' != gN happens by chance (it did: 15 of 64 elements of d proj_b one ulp off).  Those quantities pass bit-equal to g0 or
     inside the bars; outputs and activation gradients, which no kernel accumulates atomically, are held to the rule as stated;
  3. on D gN is non-finite: a poisoned row is not swallowed (the +Inf run is held to the I side only: with Inf the split GEMM operands
     legitimately produce NaN where the reference saturates a gate);
  4. g0 passes the sweep's `check` against the reference of the zero-filled inputs: the zero-filled run is the operator under test.
The data-movement kernels (sample gather / scatter, state reset, predicated commit, tensor copy) are tested directly, bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import nonfinite_cases as NC
import operator_sweep as SW
import test_conv_operators as TCONV
import test_token_operators as TTOK
from operator_sweep import check, dev, ids, restore_knobs, set_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

conv_bounds = SW.bounds_fixture("conv")
token_bounds = SW.bounds_fixture("token")
NAN, INF = float("nan"), float("inf")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def summed_over_rows(q):
    """parameter gradients and running statistics: sums over the rows of the batch, which the library accumulates with float atomics"""
    name = q.split("/")[-1]
    return name.startswith("stat:") or (name.startswith("grad:") and name[5:] not in ("x", "x2", "h0", "c0"))


def run_device(recipe, inp, dev, monkeypatch):
    case = NC.case_of(recipe)
    if recipe["suite"] == "conv":
        return {"cbs": TCONV.run_cbs, "cbs_dw": TCONV.run_cbs, "down": TCONV.run_down, "dwconv": TCONV.run_dwconv}[case["op"]](case, inp, dev)
    run = {"mswsa": TTOK.run_mswsa, "mswsa_part": TTOK.run_mswsa, "lstm": TTOK.run_lstm, "mask_token": TTOK.run_rows}[case["op"]]
    return run(case, inp, dev, monkeypatch)


def contain_and_propagate(recipe, dev, bounds, monkeypatch):
    S, case = NC.SUITES[recipe["suite"]], NC.case_of(recipe)
    if case["env"]:
        set_knobs(monkeypatch, case["env"])
    inp, r0, sets, _rN = NC.derive(recipe)
    zero_inp = NC.poisoned(recipe, inp, 0.0)
    g0, g0b, gN, gI = (run_device(recipe, NC.poisoned(recipe, inp, fill), dev, monkeypatch) for fill in (0.0, 0.0, NAN, INF))
    quantities = NC.TC.compared(case, sets) if recipe["suite"] == "token" else sorted(sets)
    misses = []
    for q in quantities:
        clean, dep = NC.clean_set(recipe, q, sets), sets[q][1]
        assert all(q in g and g[q].shape == clean.shape for g in (g0, g0b, gN, gI)), q
        exact = torch.equal(bits(g0[q])[clean], bits(g0b[q])[clean])
        for name, g in (("NaN", gN), ("+Inf", gI)):
            bad = int((~torch.isfinite(g[q][clean])).sum())
            if bad:
                misses.append(f"{q}: {bad} of {int(clean.sum())} independent elements are non-finite in the {name} run")
                continue
            if summed_over_rows(q) and torch.equal(bits(g[q])[clean], bits(g0[q])[clean]):
                continue
            if exact and not summed_over_rows(q):
                diff = int((bits(g[q])[clean] != bits(g0[q])[clean]).sum())
                if diff:
                    misses.append(f"{q}: {diff} independent elements of the {name} run differ from the zero-filled run, which repeats bit for bit")
            elif bool(clean.any()):
                rel = SW.measure(q, g[q][clean], g0[q][clean])[0]
                print(f"{recipe['id']:44s} {q:22s} {name:4s} run against the zero-filled one: {rel:.3e} (bar {SW.project_bar(q):.0e}, atomics)")
                if not rel <= SW.project_bar(q):
                    misses.append(f"{q}: the {name} run is {rel:.3e} from the zero-filled one on the independent elements")
        swallowed = int(torch.isfinite(gN[q][dep]).sum())
        if swallowed:
            misses.append(f"{q}: {swallowed} of {int(dep.sum())} dependent elements are finite in the NaN run")
        print(f"{recipe['id']:44s} {q:22s} clean {int(clean.sum()):7d}  dependent {int(dep.sum()):7d}  {'zero-filled runs bit-equal' if exact else 'zero-filled runs differ'}")
    assert not misses, f"{recipe['id']}:\n  " + "\n  ".join(misses)
    # the zero-filled run is the operator under test: the sweep's own comparison, with the reference of the zero-filled inputs
    exact_q = S.EXACT.get(case["op"], ()) if recipe["suite"] == "token" else ()
    r32 = S.reference(case, zero_inp, torch.float32) if exact_q else None
    check(S, case, g0, r0, bounds, quantities=quantities, bit_equal={q: r32[q] for q in exact_q})


@pytest.mark.parametrize("recipe", NC.CONV_RECIPES, ids=ids(NC.CONV_RECIPES))
def test_conv_operators_contain_and_propagate(recipe, dev, conv_bounds, monkeypatch):
    """conv + BatchNorm + SiLU (dense, two-source, depth-wise; strides 1, 2, 4), downsample + LayerNorm and the depth-wise conv with a
    poisoned last sample: the other samples are clean outside batch-statistics BatchNorm and every parameter gradient carries the NaN;
    with one poisoned pixel next to sample 1 in memory only the pixel's neighbourhood goes non-finite"""
    contain_and_propagate(recipe, dev, conv_bounds, monkeypatch)


@pytest.mark.parametrize("recipe", NC.TOKEN_RECIPES, ids=ids(NC.TOKEN_RECIPES))
def test_token_operators_contain_and_propagate(recipe, dev, token_bounds, monkeypatch):
    """MS-WSA with NaN in every row its selection does not keep (chain and one-kernel forward, every attention class up to T = 240,
    Context Broadcasting, DropPath): the kept rows and every parameter gradient but LN1's weight are clean; ConvLSTM with a poisoned
    sample; the mask token over poisoned rows"""
    contain_and_propagate(recipe, dev, token_bounds, monkeypatch)


# ------------------------------------------------------------------------------------------------ data movement, bit for bit
SAMPLES = [(1,), (5, 7), (8197,)]                  # tests/test_device_selection.py: unaligned rows, a scalar tail, two workgroups per row
HOST_SAMPLES = [(4096,), (8200,)]                  # the host-table kernels move whole float4 (sample sizes that are multiples of 4)
LAB = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 1, 1]], bool)      # timestep 1 selects nothing


def _features(sample, lab, seed):
    """T tensors (B, *sample): random where selected, NaN everywhere else"""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((lab.shape[1],) + sample, generator=g) for _ in range(lab.shape[0])]
    for t, x in enumerate(xs):
        x[torch.from_numpy(~lab[t])] = NAN
    return xs, g


@pytest.mark.parametrize("sample", HOST_SAMPLES, ids=lambda s: "x".join(map(str, s)))
def test_gather_samples_never_reads_an_unselected_sample(dev, sample):
    from sast_amd import functional as SF
    xs_cpu, g = _features(sample, LAB, 7)
    idx = [[b for b in range(LAB.shape[1]) if LAB[t, b]] for t in range(LAB.shape[0])]
    xs = [x.to(dev).requires_grad_(True) for x in xs_cpu]
    out = SF.gather_samples(xs, idx)
    want = torch.cat([x[i] for x, i in zip(xs_cpu, idx) if i])
    assert bool(torch.isfinite(want).all()) and torch.equal(bits(out), bits(want))
    w = torch.randn(out.shape, generator=g)
    out.backward(w.to(dev))
    rows = iter(w)
    for t, x in enumerate(xs):
        for b in range(LAB.shape[1]):
            assert torch.equal(bits(x.grad[b]), bits(next(rows) if LAB[t, b] else torch.zeros(sample))), (t, b)


@pytest.mark.parametrize("sample", SAMPLES, ids=lambda s: "x".join(map(str, s)))
def test_gather_samples_dev_never_reads_an_unselected_sample_or_row(dev, sample):
    """forward: NaN in every unselected sample; backward: NaN in the rows of the incoming gradient behind n_sel, which belong to no pair"""
    from sast_amd import functional as SF
    xs_cpu, g = _features(sample, LAB, 7)
    T, B = LAB.shape
    K = int(LAB.sum())
    sel = SF.SelectionTable(T, B, K + 2, dev).update(torch.from_numpy(LAB).to(dev))
    xs = [x.to(dev).requires_grad_(True) for x in xs_cpu]
    out = SF.gather_samples_dev(xs, sel)
    want = torch.cat([x[torch.from_numpy(LAB[t])] for t, x in enumerate(xs_cpu)])
    assert bool(torch.isfinite(want).all()) and torch.equal(bits(out[:K]), bits(want))
    assert torch.equal(bits(out[K:]), torch.zeros((2,) + sample, dtype=torch.int32))          # exact zeros behind n_sel
    w = torch.randn(out.shape, generator=g)
    w[K:] = NAN
    out.backward(w.to(dev))
    rows = iter(w[:K])
    for t, x in enumerate(xs):
        for b in range(B):
            assert torch.equal(bits(x.grad[b]), bits(next(rows) if LAB[t, b] else torch.zeros(sample))), (t, b)


def _states(sample, B, flags, seed):
    """(B, *sample): NaN in the flagged samples and in the first unflagged one, random elsewhere"""
    x = torch.randn((B,) + sample, generator=torch.Generator().manual_seed(seed))
    x[flags] = NAN
    x[int((~flags).nonzero()[0])] = NAN
    return x


FLAGS = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)


@pytest.mark.parametrize("sample", HOST_SAMPLES, ids=lambda s: "x".join(map(str, s)))
def test_zero_samples_resets_a_diverged_state_to_exact_zeros(dev, sample):
    from sast_amd import functional as SF
    cpu = _states(sample, len(FLAGS), FLAGS, 11)
    got = SF.zero_samples(cpu.to(dev), FLAGS)
    assert torch.equal(bits(got)[FLAGS], torch.zeros_like(bits(cpu)[FLAGS]))
    assert torch.equal(bits(got)[~FLAGS], bits(cpu)[~FLAGS]) and bool(torch.isnan(got[1]).all())      # the unflagged NaN sample is untouched


def test_zero_samples_dev_resets_a_diverged_state_to_exact_zeros(dev):
    """the three sample sizes as three tensors of ONE launch"""
    from sast_amd import functional as SF
    cpu = [_states(s, len(FLAGS), FLAGS, 11 + i) for i, s in enumerate(SAMPLES)]
    got = SF.zero_samples_dev([x.to(dev) for x in cpu], FLAGS.to(dev))
    for x, y in zip(cpu, got):
        assert torch.equal(bits(y)[FLAGS], torch.zeros_like(bits(x)[FLAGS]))
        assert torch.equal(bits(y)[~FLAGS], bits(x)[~FLAGS]) and bool(torch.isnan(y[1]).all())


def test_commit_samples_dev_overwrites_nan_and_never_reads_an_unflagged_sample(dev):
    """destination: NaN where it is about to be overwritten; source: NaN where it is not flagged"""
    from sast_amd import functional as SF
    B = len(FLAGS)
    g = torch.Generator().manual_seed(13)
    dst_cpu = [torch.randn((B,) + s, generator=g) for s in SAMPLES]
    src_cpu = [torch.randn((B,) + s, generator=g) for s in SAMPLES]
    for d, s in zip(dst_cpu, src_cpu):
        d[FLAGS] = NAN
        s[~FLAGS] = NAN
    got = SF.commit_samples_dev([d.to(dev) for d in dst_cpu], [s.to(dev) for s in src_cpu], FLAGS.to(dev))
    for d, s, y in zip(dst_cpu, src_cpu, got):
        assert bool(torch.isfinite(y).all())
        assert torch.equal(bits(y)[FLAGS], bits(s)[FLAGS]) and torch.equal(bits(y)[~FLAGS], bits(d)[~FLAGS])


def test_copy_tensors_moves_every_bit_over_nan(dev):
    """destinations full of NaN; the sources carry NaN, +Inf and -Inf of their own, which arrive as they are"""
    from sast_amd import functional as SF
    g = torch.Generator().manual_seed(17)
    src_cpu = [torch.randn((5,) + s, generator=g) for s in SAMPLES]
    for s in src_cpu:
        s.view(-1)[::3] = torch.tensor([NAN, INF, -INF]).repeat(math.ceil(s.numel() / 9))[:s.view(-1)[::3].numel()]
    src = [s.to(dev) for s in src_cpu]
    dst = [torch.full_like(s, NAN) for s in src]
    SF.copy_tensors(dst, src)
    for d, s in zip(dst, src_cpu):
        assert torch.equal(bits(d), bits(s))
