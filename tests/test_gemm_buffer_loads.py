"""The buffer-load addressing of the GEMM loaders (sast_amd/csrc/gemm.cuh, "BUFFERED loaders"): a slot is a 32-bit byte offset into a
buffer resource and the hardware range check replaces the address select of the zero page.  A wrong resource or offset shows as zeros or
as a neighbour's data, so every operand here is a contiguous view INSIDE a larger buffer of NaN (guard elements before and after) and
every output is pre-filled with NaN: a stray read poisons the result, a missed tile leaves NaN behind.

References are fp64 on the CPU, one per case; the bounds are those of tests/test_gemm_template.py for the same entry points (5e-6 of
the result's max-norm: the fp32 accumulation error).  The reference side is checked alone first: finite, and an fp32 evaluation of the
same expression on the CPU within the same bound of it.  The second half of the file runs the conv, stem, MS-WSA and ConvLSTM operators
on guarded inputs (their outputs are allocated by the wrappers, so only the inputs can be guarded there)."""
import ctypes as C

import pytest
import torch

from conftest import record_error
from test_gemm_template import NT_TILES, TN_TILES

pytestmark = pytest.mark.gpu

GUARD = 64                 # floats of NaN on either side of an operand (a multiple of 4: the 16-byte alignment of the rows is kept)
BOUND = 5e-6               # tests/test_gemm_template.py
SAST_EINVAL = -22


@pytest.fixture(scope="module")
def tools():
    from sast_amd import _lib as L
    lib = L.tools_lib()
    lib.sast_test_gemm_nt.restype = C.c_int
    lib.sast_test_gemm_nt.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
    lib.sast_test_gemm_tn.restype = C.c_int
    lib.sast_test_gemm_tn.argtypes = [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p]
    return lib


def guarded(t, dev):
    """a copy of `t` on the device as a contiguous view inside a NaN-filled buffer; returns (view, whole buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype, device=dev)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guarded_out(shape, dev, fill):
    """an output inside a NaN buffer, itself filled with `fill` (NaN for stores, 0 for atomic accumulation)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return view, buf


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def reference_ok(ref64, ref32):
    assert bool(torch.isfinite(ref64).all())
    err = float((ref32.double() - ref64).abs().max() / ref64.abs().max())
    assert err <= BOUND, ("the fp32 reference alone misses the bound", err)


_NT_REF, _TN_REF = {}, {}


def nt_case(shape):
    if shape not in _NT_REF:
        M, N, K = shape
        g = torch.Generator(device="cpu").manual_seed(7 * M + 3 * N + K)
        a, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        ref = a.double() @ w.double().t() + b.double()
        reference_ok(ref, a @ w.t() + b)
        _NT_REF[shape] = (a, w, b, ref)
    return _NT_REF[shape]


def tn_case(shape):
    if shape not in _TN_REF:
        Mo, NJ, R = shape
        g = torch.Generator(device="cpu").manual_seed(5 * Mo + 11 * NJ + R)
        dy, x = torch.randn(R, Mo, generator=g), torch.randn(R, NJ, generator=g)
        ref, ref_cs = dy.double().t() @ x.double(), dy.double().sum(0)
        reference_ok(ref, dy.t() @ x)
        reference_ok(ref_cs, dy.sum(0))
        _TN_REF[shape] = (dy, x, ref, ref_cs)
    return _TN_REF[shape]


@pytest.mark.parametrize("shape", [(61, 33, 48), (130, 200, 1000)])
def test_nt_guarded_operands_vs_fp64(tools, shape):
    """reduce-contiguous A and B (LdRows, LdWeightNT): no shape is a multiple of a tile, K leaves a partial last k-tile and k-groups with
    unequal tile counts -- the per-lane tail select and the invalid rows / columns folded into the base offset"""
    M, N, K = shape
    dev = torch.device("cuda:0")
    a, w, b, ref = nt_case(shape)
    (da, _), (dw, _), (db, _) = guarded(a, dev), guarded(w, dev), guarded(b, dev)
    ref = ref.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for tile in NT_TILES:
        c, cbuf = guarded_out((M, N), dev, float("nan"))
        assert tools.sast_test_gemm_nt(da.data_ptr(), dw.data_ptr(), db.data_ptr(), c.data_ptr(), M, N, K, tile, st) == 0, tile
        torch.cuda.synchronize()
        assert bool(torch.isfinite(c).all()), ("NaN in the output: a stray read or a missed tile", tile, shape)
        assert guards_intact(cbuf), ("store outside the output", tile, shape)
        err = float((c.double() - ref).abs().max() / ref.abs().max())
        print(f"nt tile {tile} shape {shape}: {err:.3e}")
        record_error("test_nt_guarded_operands_vs_fp64", f"tile {tile} shape {shape}", err, 1.0, BOUND)
        assert err <= BOUND, (tile, shape, err)


@pytest.mark.parametrize("shape", [(72, 200, 1003), (132, 36, 250)])
def test_tn_guarded_operands_with_column_sums_vs_fp64(tools, shape):
    """index-contiguous A and B (LdRowsT twice) with a reduction of 1003 / 250 rows, splits 1 and 3: the reduction tail is the path whose
    select is gone -- rows at or beyond a work item's range end must read zeros by the range check of the resource alone"""
    Mo, NJ, R = shape
    dev = torch.device("cuda:0")
    dy, x, ref, ref_cs = tn_case(shape)
    (ddy, _), (dx, _) = guarded(dy, dev), guarded(x, dev)
    ref, ref_cs = ref.to(dev), ref_cs.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for tile in TN_TILES:
        for splits in (1, 3):
            out, obuf = guarded_out((Mo, NJ), dev, 0.0)
            cs, csbuf = guarded_out((Mo,), dev, 0.0)
            assert tools.sast_test_gemm_tn(ddy.data_ptr(), dx.data_ptr(), out.data_ptr(), cs.data_ptr(), Mo, NJ, R, tile, splits, 0, st) == 0, tile
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cs).all()), ("NaN: a stray read", tile, splits, shape)
            assert guards_intact(obuf) and guards_intact(csbuf), ("atomic outside the output", tile, splits, shape)
            err = float((out.double() - ref).abs().max() / ref.abs().max())
            err_cs = float((cs.double() - ref_cs).abs().max() / ref_cs.abs().max())
            print(f"tn tile {tile} splits {splits} shape {shape}: {err:.3e} column sums {err_cs:.3e}")
            record_error("test_tn_guarded_operands_with_column_sums_vs_fp64", f"tile {tile} splits {splits} shape {shape}", err, 1.0, BOUND)
            assert err <= BOUND, (tile, splits, shape, err)
            assert err_cs <= BOUND, ("column sums", tile, splits, shape, err_cs)


def test_operand_span_beyond_2_31_bytes_is_refused(tools):
    """32-bit offsets: an operand whose addressed span reaches 2^31 bytes is SAST_EINVAL before any launch (include/sast_hip.h, size
    limits) -- the output keeps its NaN fill.  The operands are torch.empty: nothing may read them."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    K, N = 512, 32
    M = (1 << 31) // (4 * K) + 8                          # (M - 1) * K + K floats > 2^31 bytes
    a = torch.empty(M * K, device=dev)
    w = torch.empty(N, K, device=dev)
    b = torch.zeros(N, device=dev)
    c = torch.full((64, N), float("nan"), device=dev)     # nothing may be written: a window of the output is enough to see it
    for tile in (0, 19):
        assert tools.sast_test_gemm_nt(a.data_ptr(), w.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, tile, st) == SAST_EINVAL
    # the index-contiguous form: (R + slack) rows of Mo floats
    Mo, NJ = 512, 32
    R = (1 << 31) // (4 * Mo)
    x = torch.empty(R * NJ, device=dev)
    out = torch.full((Mo, NJ), float("nan"), device=dev)
    cs = torch.full((Mo,), float("nan"), device=dev)
    for splits in (1, 3):
        assert tools.sast_test_gemm_tn(a.data_ptr(), x.data_ptr(), out.data_ptr(), cs.data_ptr(), Mo, NJ, R, 50, splits, 0, st) == SAST_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(cs).all())


# ------------------------------------------------------------------------------------------------ the operators that reach the other loaders
# The conv, stem, MS-WSA and ConvLSTM operators on new small cases, called the way tests/test_conv_operators.py and
# tests/test_token_operators.py call them, with every input tensor inside a NaN-filled buffer.  Bounds: the recipe of those sweeps
# (operator_sweep.check): FACTOR x max(e32 of the case, the operator's median e32 of the committed bounds file), capped by the
# project's bars, where e32 is the float32 CPU evaluation of the reference against its float64 evaluation -- taken here, once per case.
import conv_cases as CC                                                                            # noqa: E402
import operator_sweep as SW                                                                        # noqa: E402
import token_cases as TC                                                                           # noqa: E402
from operator_sweep import check, dev, grads_of, restore_knobs  # noqa: E402,F401  (dev, restore_knobs: fixtures)


def guarded_dev_leaves(inp, dev, no_grad, grads=True, channels_last_weights=False):
    """operator_sweep.dev_leaves with every tensor a view inside a NaN buffer (uint8: a buffer of 255)"""
    out = {}
    for k, v in inp.items():
        t = v.clone()
        cl = channels_last_weights and t.dim() == 4 and k.split(".")[-1] == "w"
        phys = t.permute(0, 2, 3, 1).contiguous() if cl else t.contiguous()
        fill = 255 if phys.dtype == torch.uint8 else float("nan")
        buf = torch.full((phys.numel() + 2 * GUARD,), fill, dtype=phys.dtype, device=dev)
        view = buf[GUARD:GUARD + phys.numel()].view(phys.shape)
        view.copy_(phys)
        t = view.permute(0, 3, 1, 2) if cl else view
        if grads and t.dtype == torch.float32 and not SW._no_grad(k, no_grad):
            t.requires_grad_(True)
        out[k] = t
    return out


_OP_REF = {}


def op_reference(suite, case, inp_of=None):
    """(inputs, float64 reference, bounds document for operator_sweep.check) of a new case; the reference side is checked alone"""
    if case["id"] not in _OP_REF:
        inp = suite.make_inputs(case)
        if inp_of is not None:
            inp = inp_of(inp)
        r64, r32 = suite.reference(case, inp, torch.float64), suite.reference(case, inp, torch.float32)
        e32 = {}
        for q in suite.float_quantities(r64):
            assert bool(torch.isfinite(r64[q]).all()), (case["id"], q)
            e32[q] = SW.measure(q, r32[q], r64[q])[0]
            assert e32[q] <= SW.project_bar(q), ("the fp32 reference alone misses the project bar", case["id"], q, e32[q])
        name = "conv" if suite is CC else "token"
        _OP_REF[case["id"]] = (inp, r64, {"cases": {suite.bounds_id(case): e32}, "operators": SW.load_bounds(name)["operators"]})
    return _OP_REF[case["id"]]


CONV_UNIT_CASES = [CC._cbs(3, s, (2, 5, 7), cin, cout, modes="t") for s in (1, 2) for cin, cout in ((16, 32), (12, 20))]


@pytest.mark.parametrize("case", CONV_UNIT_CASES, ids=[c["id"] for c in CONV_UNIT_CASES])
def test_conv_unit_guarded_inputs(case, dev, monkeypatch):
    """3x3 conv + BatchNorm + SiLU, forward and the dW || dX pair: 16 -> 32 channels take the uniform-tap loaders (LdIm2colU, LdConvDxU,
    LdWeightConvDxU), 12 -> 20 the general ones; the image borders of 5 x 7 pixels and the parity classes of stride 2 are the edges"""
    import test_conv_operators as TCO
    inp, ref, bounds = op_reference(CC, case)
    monkeypatch.setattr(SW, "dev_leaves", guarded_dev_leaves)
    got = TCO.run_cbs(case, inp, dev)
    check(CC, case, got, ref, bounds)


def _stem_events(kind):
    def of(inp):
        g = SW.gen("stem-events-" + kind)
        x = ((torch.rand(inp["x"].shape, generator=g) < 0.15) * torch.randint(1, 256, inp["x"].shape, generator=g)).float()
        if kind == "one257":
            x[0, 3, 5, 7] = 257.0          # 257 = 0x43808000: not one bf16
        return dict(inp, x=x)
    return of


@pytest.mark.parametrize("kind", ["exact", "one257", "u8"])
def test_stem_guarded_inputs(kind, dev):
    """the stem conv (7x7 stride 4, replicate padding, 20 -> 64 channels, B = 2, 16 x 24 pixels) on fp32 event counts with the word that
    input_prep publishes for them -- 0: every value is one bf16, the three-term k-loop; non-zero (one value of 257): the six-term loop --
    and on the stored uint8 tensor (the 4-byte buffer loads)"""
    from sast_amd import functional as SF
    base = CC._down(4, True, (2, 16, 24), 20, 64, u8=kind == "u8")
    case = dict(base, id=base["id"] + "-" + kind)
    inp, ref, bounds = op_reference(CC, case, None if kind == "u8" else _stem_events(kind))
    p = guarded_dev_leaves(inp, dev, CC.NO_GRAD, channels_last_weights=True)
    if kind != "u8":
        p["x"].sast_nonexact = torch.full((1,), int(kind == "one257"), dtype=torch.int32, device=dev)
    y = SF.downsample_ln(p["x"], p["w"], p["ln_w"], p["ln_b"], p.get("pe"), case["f"])
    got = {"train/out:y": y.detach().cpu()}
    (y * p["g"]).sum().backward()
    grads_of(got, p, "train/")
    torch.cuda.synchronize()
    check(CC, case, got, ref, bounds)


def test_mswsa_layer_guarded_inputs(dev, monkeypatch):
    """one MS-WSA layer, forward and backward, C = 64, two partitions of 60 tokens of which 60 and 33 are kept: the gathered loaders and
    device-side row counts (dM / dR = 93) below the launched grid (120 rows)"""
    import test_token_operators as TTO
    case = TC._mswsa(64, sel="part60", tag="guarded", op="mswsa_part", B=1, N=2, T=60, peaked=False)
    assert [len(v) for _w, v in sorted(TC.kept_slots(case).items())] == [60, 33]
    inp, ref, bounds = op_reference(TC, case)
    monkeypatch.setattr(SW, "dev_leaves", guarded_dev_leaves)
    got = TTO.run_mswsa(case, inp, dev, monkeypatch)
    check(TC, case, got, ref, bounds, quantities=TC.compared(case, ref))


@pytest.mark.parametrize("state", ["given", "none"])
def test_conv_lstm_guarded_inputs(state, dev, monkeypatch):
    """ConvLSTM forward and backward, C = 64, 2 x 30 rows, with h0 given (the dual-source loaders LdRows2 / LdRowsT2 next to the buffered
    LdRowsT / LdRows / LdWeightNN of the same launches) and with None"""
    import test_token_operators as TTO
    monkeypatch.setattr(TC, "LSTM_HW", (5, 6))
    base = TC._lstm(64, state)
    case = dict(base, id=base["id"] + "-2x30")
    inp, ref, bounds = op_reference(TC, case)
    assert inp["x"].shape == (2, 5, 6, 64)
    monkeypatch.setattr(SW, "dev_leaves", guarded_dev_leaves)
    got = TTO.run_lstm(case, inp, dev, monkeypatch)
    check(TC, case, got, ref, bounds, quantities=TC.compared(case, ref))
