"""What the six fp64 operator sweeps (conv, token path, YOLOX head, optimizer, window attention, elementwise arithmetic) share: the project's bars and the error measure, the helpers of
the case modules, the generator of the fp32 bounds files, the GPU-side fixtures and the one `check` every device result goes through.

A suite is its case module (tests/conv_cases.py, token_cases.py, head_cases.py, optim_cases.py, attn_cases.py, act_cases.py), reached by name
through `suite("conv" | "token" | "head" | "optim" | "attn" | "act")`.
Generic code asks a suite for: ALL_CASES, BY_ID, make_inputs(case), reference(case, inputs, dtype), pool_key(quantity), bounds_id(case)
(the case whose bounds entry this one shares), BOUNDS_CASES (the cases with an entry of their own), float_quantities(reference) (the
compared float quantities, sorted) and DISCRETE (quantities that hold assignments, equal in every precision).

Importing this module needs neither the library nor a GPU; the fixtures import the library when a test uses them.
"""
import importlib
import json
import os
import platform
import statistics
import zlib

import pytest
import torch

from parity_helpers import _test_id

FWD_ATOL = 3e-5       # the project's bars
GRAD_RTOL = 3e-4
FACTOR = 8.0          # over max(fp32 error of the reference, operator median): another summation order of the same expression
SAST_EINVAL = -22

SUITES = ("conv", "token", "head", "optim", "attn", "act")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def suite(name):
    assert name in SUITES, name
    return importlib.import_module(name + "_cases")


def measure(quantity, got, ref):
    """(error figure the bounds are stated in, absolute max error, scale): outputs absolute (scale 1), everything else relative to the
    reference tensor's max-norm"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (quantity, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    if "out:" in quantity:
        return err, err, 1.0
    scale = float(ref.abs().max()) + 1e-30
    return err / scale, err, scale


def project_bar(quantity):
    return FWD_ATOL if "out:" in quantity else GRAD_RTOL


# ------------------------------------------------------------------------------------------------ helpers of the case modules
def gen(seed_text):
    return torch.Generator().manual_seed(zlib.crc32(seed_text.encode()))


def up(g, *shape):
    return torch.randn(*shape, generator=g) + 0.5


def _no_grad(name, no_grad):
    """`no_grad` lists full names ("drop.mlp") and last components ("run_mean" of "u1.run_mean")"""
    return name in no_grad or name.split(".")[-1] in no_grad


def leaves(inp, dtype, no_grad, grads=True):
    """the inputs of a reference evaluation in `dtype`; those that are no upstream gradient, statistic or mask are autograd leaves"""
    out = {}
    for k, v in inp.items():
        if v.dtype == torch.uint8:
            out[k] = v
            continue
        t = v.to(dtype).clone()
        if grads and not _no_grad(k, no_grad):
            t.requires_grad_(True)
        out[k] = t
    return out


def grads(out, p, prefix="", only=None):
    for k, v in p.items():
        if v.requires_grad and (only is None or k in only):
            out[f"{prefix}grad:{k}"] = v.grad if v.grad is not None else torch.zeros_like(v)


# ------------------------------------------------------------------------------------------------ the bounds files
def bounds_path(suite_name):
    return os.path.join(GOLDEN, f"{suite_name}_operator_bounds.json")


def load_bounds(suite_name):
    with open(bounds_path(suite_name)) as f:
        return json.load(f)


def evaluate(S, threads):
    torch.set_num_threads(threads)
    cases = {}
    for case in S.BOUNDS_CASES:
        inp = S.make_inputs(case)
        r64, r32 = S.reference(case, inp, torch.float64), S.reference(case, inp, torch.float32)
        qs = S.float_quantities(r64)
        assert qs == S.float_quantities(r32)
        for q in S.DISCRETE:      # the figures mean something only where both precisions reach the same assignment
            assert q not in r64 or torch.equal(r64[q], r32[q]), (case["id"], q)
        cases[case["id"]] = {q: measure(q, r32[q], r64[q])[0] for q in qs}
    return cases


def summarise(S, cases):
    pools = {}
    for cid, qs in cases.items():
        for q, e in qs.items():
            pools.setdefault(S.BY_ID[cid]["op"], {}).setdefault(S.pool_key(q), []).append(e)
    return {op: {q: {"median": statistics.median(v), "worst": max(v), "n": len(v)} for q, v in sorted(qs.items())} for op, qs in sorted(pools.items())}


def generate(suite_name, threads=(1, 4)):
    """{"cases": .., "operators": ..} of a bounds file: every figure the largest over the thread counts, printed to four digits"""
    S = suite(suite_name)
    before = torch.get_num_threads()
    try:
        runs = [evaluate(S, int(t)) for t in threads]
    finally:
        torch.set_num_threads(before)
    cases = {cid: {q: max(r[cid][q] for r in runs) for q in runs[0][cid]} for cid in runs[0]}
    doc = {"cases": cases, "operators": summarise(S, cases)}
    return json.loads(json.dumps(doc), parse_float=lambda s: float(f"{float(s):.4e}"))


def fingerprint():
    """what the fp32 figures depend on besides the expressions: the torch build, the vector ISA its CPU kernels take, the CPU model"""
    cpu = platform.machine()
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((line.split(":", 1)[1].strip() for line in f if line.startswith("model name")), cpu)
    except OSError:
        pass
    return {"torch": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability(), "cpu": cpu}


def write_bounds(doc, path):
    with open(path, "w") as f:
        json.dump(dict(doc, generated_with=fingerprint()), f, indent=1, sort_keys=True)
        f.write("\n")


# ------------------------------------------------------------------------------------------------ GPU-side fixtures and helpers
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from sast_amd import functional as SF
    assert not SF._DW_DEFER and not SF.AUTOGRAD_GRADS         # parameter gradients are accumulated in place into .grad
    return torch.device("cuda:0")


def bounds_fixture(suite_name):
    @pytest.fixture(scope="module")
    def bounds():
        return load_bounds(suite_name)
    return bounds


@pytest.fixture(autouse=True)
def restore_knobs(monkeypatch):
    """library knobs a test set through the environment are gone, and re-read, when it ends"""
    yield
    from sast_amd import _lib as SL
    monkeypatch.undo()
    SL.reload_knobs()


def set_knobs(monkeypatch, env):
    """SAST_* knobs for the next launches, through the environment (None: unset); `restore_knobs` puts everything back"""
    from sast_amd import _lib as SL
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    SL.reload_knobs()
    for k, v in env.items():
        assert v is None or SL.lib().sast_config_get(k.encode(), -12345) == int(v), k


def ids(cases):
    return [c["id"] for c in cases]


def channels_last(w):
    """logical [Cout, Cin, k, k] stored [Cout][k][k][Cin]"""
    return w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def dev_leaves(inp, dev, no_grad, grads=True, channels_last_weights=False):
    out = {}
    for k, v in inp.items():
        t = v.clone()
        if channels_last_weights and t.dim() == 4 and k.split(".")[-1] == "w":
            t = channels_last(t)
        t = t.to(dev)
        if grads and t.dtype == torch.float32 and not _no_grad(k, no_grad):
            t.requires_grad_(True)
        out[k] = t
    return out


def grads_of(out, p, prefix=""):
    for k, v in p.items():
        if v.requires_grad:
            assert v.grad is not None, f"{prefix}{k}: no gradient arrived"
            out[f"{prefix}grad:{k}"] = v.grad.detach().cpu()


def check(suite, case, got, ref, bounds, *, quantities=None, bit_equal=None, discrete=()):
    """every compared quantity of the reference against `got`, both bars; prints each figure, fails at the end with all misses.
    suite: the case module.  quantities: restricts the comparison (default: every float quantity of `ref`).  bit_equal: {quantity: the
    float32 reference tensor it must equal bit for bit} (copies and single adds).  discrete: quantities that must equal `ref` entry by
    entry (assignments)."""
    from conftest import record_error
    bit_equal = bit_equal or {}
    cid, misses = suite.bounds_id(case), []
    for q in suite.float_quantities(ref):
        if quantities is not None and q not in quantities:
            continue
        assert q in got, f"{case['id']}: the run produced no '{q}'"
        assert bool(torch.isfinite(got[q]).all()), f"{case['id']}: {q} has non-finite values"
        rel, err, scale = measure(q, got[q], ref[q])
        e32 = bounds["cases"][cid][q]
        med = bounds["operators"][case["op"]][suite.pool_key(q)]["median"]
        tol = min(project_bar(q), FACTOR * max(e32, med))
        if q in bit_equal:
            tol = 0.0
            if not torch.equal(got[q], bit_equal[q]):
                misses.append(f"{q}: not bit-equal to the float32 reference (max difference {float((got[q] - bit_equal[q]).abs().max()):.3e})")
        elif not rel <= tol:
            misses.append(f"{q}: {rel:.3e} > {tol:.3e} (e32 {e32:.3e}, operator median {med:.3e}, project bar {project_bar(q):.0e})")
        record_error(_test_id(), q, err, scale, tol)
        print(f"{case['id']:48s} {q:28s} err {rel:.3e}  e32 {e32:.3e}  median {med:.3e}  bound {tol:.3e}  ({rel / max(e32, med, 1e-30):.2f} x)")
    for q in discrete:
        if q in ref:
            assert q in got, f"{case['id']}: the run produced no '{q}'"
            if not torch.equal(got[q], ref[q]):
                misses.append(f"{q}: {int((got[q] != ref[q]).sum())} entries differ from the reference")
    assert not misses, f"{case['id']}:\n  " + "\n  ".join(misses)
