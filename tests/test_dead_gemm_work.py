"""GEMM work whose result is known beforehand is skipped, and the numbers stay what they were.

ConvLSTM from a zero cell state (`c0 is None`): c1 = f * 0 + i * (g * d) and d(f) = dc * 0 * f * (1 - f) do not depend on the forget
gate, so `sast_lstm_fwd` / `sast_lstm_bwd` run on the three live gates (SAST_LSTM_SKIP_DEAD_GATE, default 1).  The skipping path is
compared with the FULL four-gate path on the same inputs with an explicit all-zero c0 tensor (knob 0 as well):

  * h1, c1, dx, dh0: no atomics -- torch.equal;
  * dw, db: split-R jobs that accumulate with float atomics.  The test makes the accumulation deterministic (SAST_TN_BLOCKS_PAIRED=1:
    one workgroup per output tile, one add per element onto the buffer) and requires equality there too; the rows [0, C) of both (the
    forget gate's) must come back bit for bit as the sentinel values the buffers held before the call.  With the default split counts
    the run-to-run spread of the full path and the skip-vs-full difference are PRINTED (test_lstm_atomic_spread_figures), not asserted:
    equality under the deterministic setting is the stronger statement.
"""
import ctypes as C

import pytest
import torch

import operator_sweep as SW
from operator_sweep import FACTOR, SAST_EINVAL, dev, restore_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

KNOB = "SAST_LSTM_SKIP_DEAD_GATE"
DET = "SAST_TN_BLOCKS_PAIRED"


@pytest.fixture()
def knobs(monkeypatch):
    """knobs(**env) changes SAST_* knobs for the next launches (None: unset); `restore_knobs` puts everything back afterwards"""
    return lambda **env: SW.set_knobs(monkeypatch, env)


def _lstm_inputs(dev, C_, rows, h0_given, drop_given, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 7 * C_ + rows)
    shape = (2, rows // 2, C_)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).to(dev)

    d = {"x": rnd(*shape), "h0": rnd(*shape) if h0_given else None,
         "drop": ((torch.rand(*shape, generator=g) > 0.25).float() / 0.75).to(dev) if drop_given else None,
         "w": rnd(4 * C_, 2 * C_, scale=(2 * C_) ** -0.5), "b": rnd(4 * C_, scale=0.1),
         "dh": rnd(*shape), "dhb": rnd(*shape), "dc": rnd(*shape),
         "gw": rnd(4 * C_, 2 * C_), "gb": rnd(4 * C_)}          # what the accumulate-into gradient buffers hold before the call
    return d


def _lstm_run(d, c0):
    """one forward + backward of functional.conv_lstm (two handles on h1, both with a gradient) -> dict of results"""
    from sast_amd import functional as SF
    x = d["x"].clone().requires_grad_(True)
    h0 = d["h0"].clone().requires_grad_(True) if d["h0"] is not None else None
    w, b = d["w"].clone().requires_grad_(True), d["b"].clone().requires_grad_(True)
    w.grad, b.grad = d["gw"].clone(), d["gb"].clone()
    h1, h1b, c1 = SF.conv_lstm(x, h0, c0, w, b, two_h=True, drop_mask=d["drop"])
    outs, grads = [h1, c1], [d["dh"], d["dc"]]
    if h1b is not h1:
        outs.append(h1b)
        grads.append(d["dhb"])
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    return {"h1": h1.detach(), "c1": c1.detach(), "dx": x.grad, "dh0": h0.grad if h0 is not None else None, "dw": w.grad, "db": b.grad}


LSTM_CASES = [(C_, rows, h0, drop) for C_ in (64, 128, 256, 512) for rows in (960, 950) for h0 in (False, True) for drop in (False, True)]


@pytest.mark.parametrize("C_,rows,h0_given,drop_given", LSTM_CASES)
def test_lstm_zero_cell_state_skips_the_forget_gate(dev, knobs, C_, rows, h0_given, drop_given):
    d = _lstm_inputs(dev, C_, rows, h0_given, drop_given)
    knobs(**{KNOB: 0, DET: 1})
    full = _lstm_run(d, torch.zeros_like(d["x"]))        # the four-gate path on an explicit all-zero cell state
    full_none = _lstm_run(d, None)                       # ... and on c0 = None with the knob off
    knobs(**{KNOB: 1, DET: 1})
    skip = _lstm_run(d, None)
    for k in ("h1", "c1", "dx", "dh0", "dw", "db"):
        if full[k] is None:
            assert skip[k] is None and full_none[k] is None
            continue
        assert torch.isfinite(skip[k]).all(), k
        assert torch.equal(skip[k], full[k]), (k, float((skip[k] - full[k]).abs().max()))
        assert torch.equal(full_none[k], full[k]), (k, "knob 0", float((full_none[k] - full[k]).abs().max()))
    # the forget gate's rows of the accumulate-into buffers: untouched
    assert torch.equal(skip["dw"][:C_], d["gw"][:C_]) and torch.equal(skip["db"][:C_], d["gb"][:C_])
    assert not torch.equal(skip["dw"][C_:], d["gw"][C_:]) and not torch.equal(skip["db"][C_:], d["gb"][C_:])


def test_lstm_skip_is_the_default(dev, knobs):
    """knob unset = skipping: the forward of a zero cell state launches the three-gate tile (the library's own launch profile)"""
    from sast_amd.profiling import kernel_report
    d = _lstm_inputs(dev, 64, 960, False, False)
    knobs(**{KNOB: None})
    names = " ".join(r["name"] for r in kernel_report(lambda n: [_lstm_run(d, None) for _ in range(n)], 1))
    assert "EpLstm3" in names, names
    knobs(**{KNOB: 0})
    names = " ".join(r["name"] for r in kernel_report(lambda n: [_lstm_run(d, None) for _ in range(n)], 1))
    assert "EpLstm3" not in names and "EpLstm" in names, names


@pytest.mark.parametrize("only_hidden", [True, False])
def test_lstm_dws_conv_mode_takes_the_skipping_path(dev, knobs, only_hidden):
    """dws_conv=True: the module hands the fused launch a non-NULL h0 (the depth-wise conv of the zero state) but still c0 = None"""
    from sast_amd.layers.rnn import DWSConvLSTM2d
    torch.manual_seed(3)
    m = DWSConvLSTM2d(64, dws_conv=True, dws_conv_only_hidden=only_hidden).to(dev)
    x = torch.randn(2, 64, 20, 24, device=dev)
    dh, dc = torch.randn(2, 64, 20, 24, device=dev), torch.randn(2, 64, 20, 24, device=dev)

    def run():
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        h1, c1 = m(xi)
        torch.autograd.backward([h1, c1], [dh, dc])
        torch.cuda.synchronize()
        return [h1.detach().clone(), c1.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    knobs(**{KNOB: 0, DET: 1})
    full = run()
    knobs(**{KNOB: 1, DET: 1})
    skip = run()
    for i, (a, b) in enumerate(zip(skip, full)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
    wg = m.conv1x1.weight.grad
    assert float(wg[:64].abs().max()) == 0.0 and float(wg[64:].abs().max()) > 0.0


def test_lstm_zero_state_refuses_dc0(dev, knobs):
    """c0 == NULL with dc0 != NULL needs the forget gate, which the skipping forward does not save"""
    from sast_amd import _lib as L, functional as SF
    knobs(**{KNOB: 1})
    C_, rows = 64, 128
    d = _lstm_inputs(dev, C_, rows, False, False)
    x = d["x"].contiguous()
    h1, c1, dx, dc0 = (torch.empty_like(x) for _ in range(4))
    gates, ws = torch.empty(rows, 4 * C_, device=dev), torch.empty(rows * 4 * C_, device=dev)
    dw, db = torch.zeros_like(d["w"]), torch.zeros_like(d["b"])
    a = SF._fill(L.SastLstmArgs(), B=2, L=rows // 2, C=C_, x=x, h0=None, c0=None, w=d["w"], b=d["b"], h1=h1, c1=c1, gates=gates)
    assert L.lib().sast_lstm_fwd(C.byref(a), SF._stream()) == 0
    a = SF._fill(L.SastLstmArgs(), B=2, L=rows // 2, C=C_, x=x, h0=None, c0=None, w=d["w"], b=d["b"], c1=c1, gates=gates, dh1=d["dh"],
                 dc1=None, dx=dx, dh0=None, dc0=dc0, dw=dw, db=db, ws=ws, dh1b=None, drop=None)
    assert L.lib().sast_lstm_bwd(C.byref(a), SF._stream()) == SAST_EINVAL
    a.dc0 = None
    assert L.lib().sast_lstm_bwd(C.byref(a), SF._stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()


def test_lstm_atomic_spread_figures(dev, knobs):
    """default split counts: max-norm relative difference of dw / db between 5 runs of the FULL path (float atomics in another order),
    and between the skipping and the full path.  Printed, not asserted: see the module docstring."""
    for C_, rows in ((64, 3840), (256, 3840)):
        d = _lstm_inputs(dev, C_, rows, True, False)
        knobs(**{KNOB: 0, DET: None})
        runs = [_lstm_run(d, torch.zeros_like(d["x"])) for _ in range(5)]
        knobs(**{KNOB: 1, DET: None})
        skip = _lstm_run(d, None)
        for k in ("dw", "db"):
            ref = runs[0][k] - (d["gw"] if k == "dw" else d["gb"])
            scale = float(ref.abs().max())
            pp = max(float((r[k] - runs[0][k]).abs().max()) for r in runs[1:]) / scale
            nf = float((skip[k] - runs[0][k]).abs().max()) / scale
            print(f"lstm atomic spread C={C_} rows={rows} {k}: full-vs-full (5 runs) {pp:.3e}  skip-vs-full {nf:.3e}")
            assert nf < 1e-5      # a sanity bound far above either figure: fp32 accumulation of <= 3840 terms


# ------------------------------------------------------------------------------------------------ the stem on an event tensor that is exact in bf16
# Stem: stacked-histogram counts are small integers, each exactly one bf16, so the middle and bottom planes of the operand's exact
# three-way bf16 split are zero and three of the six MFMA terms multiply zeros.  `input_prep` publishes one word per call (0 = every value
# is one bf16); while it reads 0 the stem's GEMMs stage one plane of that operand and issue three terms (SAST_STEM_EXACT_BF16, default 1).
# The conv output (seen through the LayerNorm behind it) must equal the six-term path's bit for bit; the weight gradient is a split-R job
# with float atomics: made deterministic (SAST_TN_BLOCKS=1: one workgroup per output tile) it must be equal too.
STEM_KNOB = "SAST_STEM_EXACT_BF16"
STEM_DET = "SAST_TN_BLOCKS"


def _stem_params(dev, cin=20, cout=64, f=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    k = 2 * f - 1
    w = torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5
    return {"w": w, "ln_w": 1 + 0.1 * torch.randn(cout, generator=g), "ln_b": 0.1 * torch.randn(cout, generator=g), "f": f, "seed": seed}


def _stem_run(xin, P, dev):
    """downsample_ln forward + backward on a prepared NHWC input -> (y, dw)"""
    from sast_amd import functional as SF
    w = P["w"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ln_w, ln_b = P["ln_w"].to(dev).requires_grad_(True), P["ln_b"].to(dev).requires_grad_(True)
    y = SF.downsample_ln(xin, w, ln_w, ln_b, None, P["f"])
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(P["seed"] + 1)).to(dev) + 0.5
    (y * g).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), w.grad.detach(), ln_w.grad.detach(), ln_b.grad.detach()


def _events(kind, shape, seed=11):
    g = torch.Generator().manual_seed(seed)
    if kind == "binary_i32":          # the benchmark protocol: (rand > 0.5).int()
        return (torch.rand(shape, generator=g) > 0.5).int()
    if kind == "counts_u8":
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    if kind == "counts_i32":
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
    if kind == "one_257_i32":         # 257 = 0x43808000: not one bf16
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
        x[0, 3, 5, 7] = 257
        return x
    if kind == "fractional_f32":
        return torch.rand(shape, generator=g) * 3.0
    raise AssertionError(kind)


def _kernel_names(fn):
    from sast_amd.profiling import kernel_report
    return " ".join(r["name"] for r in kernel_report(lambda n: [fn() for _ in range(n)], 1))


GEOMS = {"1mpx": ((1, 20, 384, 640), None), "gen1": ((2, 20, 240, 304), (256, 320))}


@pytest.mark.parametrize("geom", sorted(GEOMS))
@pytest.mark.parametrize("kind", ["binary_i32", "counts_u8", "counts_i32"])
def test_stem_three_term_equals_six_term(dev, knobs, geom, kind):
    from sast_amd import functional as SF
    shape, pad = GEOMS[geom]
    x = _events(kind, shape).to(dev)
    P = _stem_params(dev)

    def run():
        r, xin = SF.input_prep(x, pad, {}, keep_bytes=True)
        if xin.dtype == torch.float32:
            assert int(xin.sast_nonexact.item()) == 0, "integer counts <= 255 are exact in bf16"
        else:
            assert kind == "counts_u8" and not hasattr(xin, "sast_nonexact")
        return _stem_run(xin, P, dev)

    knobs(**{STEM_KNOB: 0, STEM_DET: 1})
    six = run()
    assert "LdExactBf16" not in _kernel_names(run)
    knobs(**{STEM_KNOB: 1, STEM_DET: 1})
    three = run()
    assert "LdExactBf16" in _kernel_names(run)
    for name, a, b in zip(("y", "dw"), three, six):       # (the LayerNorm's own parameter gradients are atomic sums of another kernel)
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


@pytest.mark.parametrize("u8", [False, True])
def test_stem_ragged_last_tile(dev, knobs, u8):
    """117 output rows per sample (not a multiple of the 64 / 32-row tiles), reached by a direct call: an integer-valued fp32 tensor with
    a word that reads 0 (what input_prep would have written), or the uint8 tensor (exact by type)"""
    shape = (3, 36, 52, 20)                       # NHWC
    xi = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    P = _stem_params(dev)

    def run():
        xin = xi.to(torch.uint8).to(dev) if u8 else xi.float().to(dev)
        if not u8:
            xin.sast_nonexact = torch.zeros(1, device=dev, dtype=torch.int32)
        return _stem_run(xin, P, dev)

    knobs(**{STEM_KNOB: 0, STEM_DET: 1})
    six = run()
    knobs(**{STEM_KNOB: 1, STEM_DET: 1})
    three = run()
    assert "LdExactBf16" in _kernel_names(run)
    for name, a, b in zip(("y", "dw"), three, six):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_stem_direct_fp32_call_without_word_stays_six_term(dev, knobs):
    """an fp32 buffer that did not come from input_prep carries no word: the loaders without the trait, whatever the values"""
    xin = torch.randint(0, 2, (2, 64, 64, 20), generator=torch.Generator().manual_seed(4)).float().to(dev)
    P = _stem_params(dev)
    knobs(**{STEM_KNOB: 1, STEM_DET: 1})
    assert "LdExactBf16" not in _kernel_names(lambda: _stem_run(xin, P, dev))
    a = _stem_run(xin, P, dev)
    knobs(**{STEM_KNOB: 0, STEM_DET: 1})
    b = _stem_run(xin, P, dev)
    for u, v in zip(a[:2], b[:2]):
        assert torch.equal(u, v)


def test_stem_three_term_body_is_the_one_that_runs(dev, knobs):
    """the word decides the body on the device: a fractional tensor handed over with a word that (wrongly) reads 0 loses its lower
    planes -- a relative error of about 2^-8 in the conv -- while the same tensor with a non-zero word gives the six-term result"""
    xf = (torch.rand(2, 64, 64, 20, generator=torch.Generator().manual_seed(6)) * 3.0).to(dev)
    P = _stem_params(dev)
    knobs(**{STEM_KNOB: 1, STEM_DET: 1})
    plain = _stem_run(xf.clone(), P, dev)
    lie, truth = xf.clone(), xf.clone()
    lie.sast_nonexact = torch.zeros(1, device=dev, dtype=torch.int32)
    truth.sast_nonexact = torch.ones(1, device=dev, dtype=torch.int32)
    y_lie, y_truth = _stem_run(lie, P, dev), _stem_run(truth, P, dev)
    assert torch.equal(y_truth[0], plain[0]) and torch.equal(y_truth[1], plain[1])
    err = float((y_lie[0] - plain[0]).abs().max())
    assert 1e-5 < err < 1e-1, err


@pytest.mark.parametrize("kind", ["one_257_i32", "fractional_f32"])
def test_stem_mixed_input_falls_back_and_matches_fp64(dev, knobs, kind):
    """one value that is not a bf16 -> the word is non-zero -> six terms; against the float64 reference of tests/conv_reference.py within
    the bounds tests/golden/conv_operator_bounds.json holds for the stem's shape class (factor 4, overlap, 20 -> 64 channels)"""
    import conv_cases as CC
    import conv_reference as R
    from sast_amd import functional as SF
    bounds = SW.load_bounds("conv")
    x = _events(kind, (2, 20, 64, 96)).to(dev)
    P = _stem_params(dev)
    knobs(**{STEM_KNOB: 1})
    r, xin = SF.input_prep(x, None, {})
    assert int(xin.sast_nonexact.item()) != 0
    y, dw, dlw, dlb = _stem_run(xin, P, dev)
    # knob 0 on the same input: the fall-back is the six-term path itself (forward: no atomics)
    knobs(**{STEM_KNOB: 0})
    assert torch.equal(_stem_run(SF.input_prep(x, None, {})[1], P, dev)[0], y)
    # float64 reference
    xr = x.permute(0, 2, 3, 1).double().cpu()
    w, lw, lb = (P[k].double().requires_grad_(True) for k in ("w", "ln_w", "ln_b"))
    yr = R.downsample_ln(xr, w, lw, lb, None, P["f"])
    g = torch.randn(yr.shape, generator=torch.Generator().manual_seed(P["seed"] + 1)) + 0.5
    (yr * g.double()).sum().backward()
    got = {"train/out:y": y, "train/grad:w": dw, "train/grad:ln_w": dlw, "train/grad:ln_b": dlb}
    ref = {"train/out:y": yr.detach(), "train/grad:w": w.grad, "train/grad:ln_w": lw.grad, "train/grad:ln_b": lb.grad}
    cid = "down-f4o-2x24x40-20to64-pe"
    for q in sorted(ref):
        rel, err, scale = SW.measure(q, got[q], ref[q])
        tol = min(SW.project_bar(q), FACTOR * max(bounds["cases"][cid][q], bounds["operators"]["down"][CC.pool_key(q)]["median"]))
        print(f"stem mixed input {kind:16s} {q:20s} err {rel:.3e}  bound {tol:.3e}")
        assert rel <= tol, (kind, q, rel, tol)


def test_stem_word_is_reevaluated_on_graph_replay(dev, knobs):
    """one captured graph (input_prep + stem), replayed on an exact event tensor and then on a fractional one written into the same static
    buffer: the second replay must see a non-zero word and give the six-term result, not the body frozen at capture time"""
    from sast_amd import functional as SF
    P = _stem_params(dev)
    w = P["w"].to(dev).contiguous(memory_format=torch.channels_last)
    ln_w, ln_b = P["ln_w"].to(dev), P["ln_b"].to(dev)
    exact = _events("counts_i32", (2, 20, 64, 64)).float().to(dev)
    frac = _events("fractional_f32", (2, 20, 64, 64)).to(dev)

    def eager(x):
        with torch.no_grad():
            r, xin = SF.input_prep(x, None, {})
            return SF.downsample_ln(xin, w, ln_w, ln_b, None, P["f"]).clone()

    knobs(**{STEM_KNOB: 0})
    want_exact, want_frac = eager(exact), eager(frac)
    knobs(**{STEM_KNOB: 1})
    static_x = exact.clone()
    cache = {}
    word = torch.full((1,), -1, device=dev, dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        SF.input_prep(static_x, None, cache)                     # un-captured warm-up: the scratch is born outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        r, xin = SF.input_prep(static_x, None, cache)
        out = SF.downsample_ln(xin, w, ln_w, ln_b, None, P["f"])
        word.copy_(xin.sast_nonexact)
    graph.replay()
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and torch.equal(out, want_exact)
    static_x.copy_(frac)
    graph.replay()
    torch.cuda.synchronize()
    assert int(word.item()) != 0 and torch.equal(out, want_frac), float((out - want_frac).abs().max())
    static_x.copy_(exact)
    graph.replay()
    torch.cuda.synchronize()
    assert int(word.item()) == 0 and torch.equal(out, want_exact)


@pytest.mark.parametrize("h0_given", [False, True])
def test_lstm_three_gate_k_split_tile(dev, knobs, h0_given):
    """SAST_LSTM_TILE=1 with a reduction of >= 256: the 4-k-group form of the three-gate tile (32 x 96) against the four-gate one"""
    from sast_amd.profiling import kernel_report
    d = _lstm_inputs(dev, 256, 950, h0_given, True)
    knobs(**{KNOB: 0, DET: 1, "SAST_LSTM_TILE": 1})
    full = _lstm_run(d, torch.zeros_like(d["x"]))
    knobs(**{KNOB: 1, DET: 1, "SAST_LSTM_TILE": 1})
    skip = _lstm_run(d, None)
    names = " ".join(r["name"] for r in kernel_report(lambda n: [_lstm_run(d, None) for _ in range(n)], 1))
    assert "Tile<32, 96, 1, 1, 3, 16, 4" in names and "EpLstm3" in names, names
    for k in ("h1", "c1", "dx", "dh0", "dw", "db"):
        if full[k] is not None:
            assert torch.equal(skip[k], full[k]), (k, float((skip[k] - full[k]).abs().max()))


def test_stem_one_word_per_event_tensor(dev, knobs):
    """two live event tensors, one exact and one not (two timesteps of a sequence), whose backwards run after BOTH forwards: each
    weight gradient must read its own tensor's word"""
    from sast_amd import functional as SF
    P = _stem_params(dev)
    xs = [_events("counts_i32", (2, 20, 64, 64)).to(dev), _events("fractional_f32", (2, 20, 64, 64)).to(dev)]

    def run():
        cache, ys, ws = {}, [], []
        for x in xs:
            r, xin = SF.input_prep(x, None, cache)
            w = P["w"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            ys.append(SF.downsample_ln(xin, w, P["ln_w"].to(dev), P["ln_b"].to(dev), None, P["f"]))
            ws.append(w)
        for y in reversed(ys):
            (y * (torch.arange(y.numel(), device=dev).view(y.shape) % 7 - 3.0)).sum().backward()
        torch.cuda.synchronize()
        return [y.detach() for y in ys] + [w.grad for w in ws]

    knobs(**{STEM_KNOB: 0, STEM_DET: 1})
    six = run()
    knobs(**{STEM_KNOB: 1, STEM_DET: 1})
    three = run()
    r0, x0 = SF.input_prep(xs[0], None, {})
    r1, x1 = SF.input_prep(xs[1], None, {})
    assert int(x0.sast_nonexact.item()) == 0 and int(x1.sast_nonexact.item()) != 0
    for i, (a, b) in enumerate(zip(three, six)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
