"""The window-attention kernels of csrc/k_attn_mfma.hip on their own (sast_test_attn_fwd / sast_test_attn_bwd of the tools library: the
launchers attn_fwd_mfma_launch / attn_bwd_mfma_launch without LayerScale side workgroups) against the float64 expression of
tests/attn_reference.py on the cases of tests/attn_cases.py: the fifth suite of tests/operator_sweep.py.

Every one of the eleven kernels (forward <2> / <3> / <4> / big, backward <2> / <2,split> / <3> / <3,split> / <4> / big_q + big_kv), every
body of their tile-count switches, K on either side of every multiple of 32 up to 128, K = 1, dropped groups, dim_head 4 .. 32 with one,
two and three heads, both values of SAST_ATTN_BWD_SPLIT, and logits of std 4 (the running maximum and the exp(m - mn) factor of the
two-sweep kernels).  Compared: o (absolute), lse, dq, dk, dv (each relative to its own max-norm), under the two bars of the other
sweeps -- the project's FWD_ATOL / GRAD_RTOL and FACTOR x max(e32 of the case, median e32 of the operator), where e32 is the error of the
float32 CPU expression against float64 (tests/golden/attn_operator_bounds.json: never a figure the kernels produced).  The backward
consumes the forward kernel's own lse, which is the product's pairing.

Memory discipline: every buffer has TAIL rows behind the last kept row.  In the inputs they are NaN (a partial tile that read past its
group would poison the result); the outputs are NaN on the kept rows (an element the kernels do not write fails the finiteness test of
`check`) and a sentinel on the tail, which must come back bit for bit.
"""
import ctypes as C

import pytest
import torch

import attn_cases as AC
import operator_sweep as SW
from operator_sweep import SAST_EINVAL, check, dev, ids, restore_knobs, set_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

bounds = SW.bounds_fixture("attn")
TAIL = 128
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def tools():
    from sast_amd import _lib as L
    lib = L.tools_lib()
    lib.sast_test_attn_fwd.restype = C.c_int
    lib.sast_test_attn_fwd.argtypes = [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]
    lib.sast_test_attn_bwd.restype = C.c_int
    lib.sast_test_attn_bwd.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p] * 2
    return lib


def _padded(t, dev, fill=float("nan")):
    """`t` on the device with TAIL rows of `fill` behind it"""
    out = torch.full((t.shape[0] + TAIL,) + tuple(t.shape[1:]), fill, dtype=torch.float32, device=dev)
    out[:t.shape[0]] = t.to(dev)
    return out


def _output(rows, cols, dev):
    """NaN on the kept rows, the sentinel on the tail"""
    out = torch.full((rows + TAIL, cols), float("nan"), device=dev)
    out[rows:] = SENTINEL
    return out


def _tail_untouched(t, rows):
    return bool((t[rows:] == SENTINEL).all())


def _groups(Ks, dev):
    Kw = torch.tensor(Ks, dtype=torch.int32)
    row_off = torch.cumsum(Kw, 0, dtype=torch.int32) - Kw
    return Kw.to(dev), row_off.to(dev)


def run_attn(tools, case, inp, dev):
    """forward, then the backward on the forward's own lse -> the suite's quantities (CPU tensors)"""
    import attn_reference as R
    from sast_amd import functional as SF
    Ks, T, Cc, dh = case["Ks"], case["T"], case["C"], case["dh"]
    rows, heads, st = sum(Ks), Cc // dh, SF._stream()
    Kw, row_off = _groups(Ks, dev)
    qkv, dout = _padded(inp["qkv"], dev), _padded(inp["dout"], dev)
    o, lse, dqkv = _output(rows, Cc, dev), _output(rows, heads, dev), _output(rows, 3 * Cc, dev)
    dbuf = torch.full((rows + TAIL, heads), float("nan"), device=dev)
    assert tools.sast_test_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), row_off.data_ptr(), Kw.data_ptr(), len(Ks), T, Cc, dh, st) == 0
    torch.cuda.synchronize()
    assert _tail_untouched(o, rows) and _tail_untouched(lse, rows), "the forward wrote behind the last kept row"
    lse_in = lse.clone()
    lse_in[rows:] = float("nan")
    assert tools.sast_test_attn_bwd(qkv.data_ptr(), dout.data_ptr(), lse_in.data_ptr(), dqkv.data_ptr(), row_off.data_ptr(), Kw.data_ptr(),
                                    len(Ks), T, Cc, dh, dbuf.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert _tail_untouched(dqkv, rows), "the backward wrote behind the last kept row"
    assert bool(torch.isnan(dbuf[rows:]).all()) and torch.equal(qkv[:rows].cpu(), inp["qkv"]) and torch.equal(dout[:rows].cpu(), inp["dout"])
    if T <= 128:
        assert bool(torch.isnan(dbuf).all()), "the one-launch backward has no use for the scratch"
    dq, dk, dv = R.split_qkv(dqkv[:rows].cpu(), dh)
    return {"out:o": o[:rows].cpu(), "rel:lse": lse[:rows].cpu(), "grad:q": dq.clone(), "grad:k": dk.clone(), "grad:v": dv.clone()}


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("case", AC.ALL_CASES, ids=ids(AC.ALL_CASES))
def test_attention(case, dev, bounds, tools, monkeypatch):
    if case["env"]:
        set_knobs(monkeypatch, case["env"])
    inp = AC.make_inputs(case)
    AC.check_conditions(case, inp)          # on the CPU, on the float64 reference, before the device run
    ref = AC.reference(case, inp, torch.float64)
    got = run_attn(tools, case, inp, dev)
    check(AC, case, got, ref, bounds)


# ------------------------------------------------------------------------------------------------ which kernel ran
FWD = {2: "attn_fwd_mfma_kernel<2>", 3: "attn_fwd_mfma_kernel<3>", 4: "attn_fwd_mfma_kernel<4>", 8: "attn_fwd_big_kernel"}
BWD = {(2, 1): {"attn_bwd_mfma_kernel<2,split>"}, (3, 1): {"attn_bwd_mfma_kernel<3,split>"}, (2, 0): {"attn_bwd_mfma_kernel<2>"},
       (3, 0): {"attn_bwd_mfma_kernel<3>"}, (4, 1): {"attn_bwd_mfma_kernel<4>"}, (4, 0): {"attn_bwd_mfma_kernel<4>"},
       (8, 1): {"attn_bwd_big_q_kernel", "attn_bwd_big_kv_kernel"}, (8, 0): {"attn_bwd_big_q_kernel", "attn_bwd_big_kv_kernel"}}


def test_every_kernel_is_reached_and_the_split_knob_selects_the_backward(dev, tools, monkeypatch):
    """the library's own launch profile (sast_amd.profiling.kernel_report) of one case per partition size of the table, under both
    values of SAST_ATTN_BWD_SPLIT: exactly the forward and backward kernels of the partition's class, the sequential <2> / <3> instead
    of the split ones under 0, <4> and the big pair under either; together all eleven"""
    from sast_amd.profiling import kernel_report
    seen = set()
    for split in (1, 0):
        set_knobs(monkeypatch, {"SAST_ATTN_BWD_SPLIT": split} if not split else {"SAST_ATTN_BWD_SPLIT": None})
        for T in AC.KS:
            case = AC.BY_ID[f"attn-t{T}-c64-dh32"]
            inp = AC.make_inputs(case)
            names = {r["name"] for r in kernel_report(lambda n: [run_attn(tools, case, inp, dev) for _ in range(n)], 1) if r["name"].startswith("attn_")}
            cls = AC.dispatch_class(T)
            assert names == {FWD[cls]} | BWD[(cls, split)], (T, split, names)
            seen |= names
    assert seen == set(FWD.values()) | set().union(*BWD.values()) and len(seen) == 11
    assert {AC.dispatch_class(c["T"]) for c in AC.ALL_CASES if c["env"] == AC.NOSPLIT} == {2, 3}       # the table runs the knob where it matters


# ------------------------------------------------------------------------------------------------ refusals
def test_launchers_refuse_bad_arguments_before_anything_runs(dev, tools):
    """dim_head 2, 6 and 36, a width that is no multiple of dim_head, T = 257, and the T > 128 backward without its scratch:
    SAST_EINVAL, and every output still at its fill"""
    from sast_amd import functional as SF
    st = SF._stream()
    for T, Cc, dh, with_dbuf, fwd_refuses in ((60, 8, 2, True, True), (60, 12, 6, True, True), (60, 72, 36, True, True), (60, 40, 16, True, True),
                                              (257, 64, 32, True, True), (129, 64, 32, False, False)):
        Ks = [min(T, 256), 5]
        rows, heads = sum(Ks), max(Cc // dh, 1)
        Kw, row_off = _groups(Ks, dev)
        qkv, dout = torch.ones(rows + TAIL, 3 * Cc, device=dev), torch.ones(rows + TAIL, Cc, device=dev)
        o, lse, dqkv = (torch.full((rows + TAIL, n), SENTINEL, device=dev) for n in (Cc, heads, 3 * Cc))
        dbuf = torch.full((rows + TAIL, heads), SENTINEL, device=dev)
        rc = tools.sast_test_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), row_off.data_ptr(), Kw.data_ptr(), len(Ks), T, Cc, dh, st)
        torch.cuda.synchronize()
        assert rc == (SAST_EINVAL if fwd_refuses else 0), (T, Cc, dh, rc)
        if fwd_refuses:
            assert bool((o == SENTINEL).all()) and bool((lse == SENTINEL).all()), (T, Cc, dh)
        else:
            assert bool(torch.isfinite(lse[:rows]).all()) and not bool((lse[:rows] == SENTINEL).any())
        lse_in = lse.clone()
        rc = tools.sast_test_attn_bwd(qkv.data_ptr(), dout.data_ptr(), lse_in.data_ptr(), dqkv.data_ptr(), row_off.data_ptr(), Kw.data_ptr(),
                                      len(Ks), T, Cc, dh, dbuf.data_ptr() if with_dbuf else None, st)
        torch.cuda.synchronize()
        assert rc == SAST_EINVAL, (T, Cc, dh, with_dbuf, rc)
        assert bool((dqkv == SENTINEL).all()) and bool((dbuf == SENTINEL).all()), (T, Cc, dh)
