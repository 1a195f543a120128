"""The mixed-density event stack (sast_amd.events.MixedDensityEventStack, representation="mixed_density" of EventFrames / EventStreams,
sast_mdstack_frames of csrc/k_events.hip) and int8 frames into the detector's input kernels.

GPU tests hold the device front end to byte equality with frames the reference produced on the CPU (tests/golden/mixed_density.npz,
written by tests/golden/make_golden_mixed_density.py); the events are regenerated from the golden modules' integer hash.  Everything is
integer: there is no tolerance anywhere.  CPU tests: the symbols (the ABI of the struct: tests/test_abi.py), argument checks, and that the numpy
restatement of the rule equals every fixture frame (which pins the restatement, used by the GPU tests for a few extra cases, to the
reference)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_events as G  # noqa: E402
import make_golden_mixed_density as M  # noqa: E402

gpu = pytest.mark.gpu

LAUNCHES_PER_CALL = 7      # the stacked-histogram call's: 2 time correction + 1 window search + 4 frames


def _fixtures():
    return np.load(os.path.join(GOLDEN, "mixed_density.npz"))


def _ref_available():
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "data", "utils", "representations.py"))


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_mdstack_entry_points_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_mdstack_")]
    assert sorted(names) == ["sast_mdstack_frames", "sast_mdstack_frames_ws_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    # the workspace query is host-only: the record area and the geometry limits
    assert lib.sast_mdstack_frames_ws_bytes(4, 20, 720, 1280, 1, 1 << 20) > 4 * (1 << 22)
    assert lib.sast_mdstack_frames_ws_bytes(1, 512, 24, 72, 0, 16) > 0
    assert lib.sast_mdstack_frames_ws_bytes(1, 513, 24, 72, 0, 16) == 0       # the record's channel field holds 2 * bin + polarity
    assert lib.sast_mdstack_frames_ws_bytes(0, 10, 24, 72, 0, 16) == 0
    assert lib.sast_mdstack_frames(None, None) != 0
    a = _lib.SastMdStackArgs()                                                 # all pointers NULL: refused before any launch
    a.B, a.bins, a.height, a.width = 1, 10, 24, 72
    assert lib.sast_mdstack_frames(C.byref(a), None) != 0


def test_mixed_density_constructor_validation():
    from sast_amd.events import EventFrames, EventStreams, MixedDensityEventStack
    rep = MixedDensityEventStack(20, 24, 72)
    assert rep.get_shape() == (20, 24, 72) and rep.count_cutoff is None
    assert rep.get_torch_dtype() == torch.int8 and rep.dtype == torch.int8
    assert MixedDensityEventStack(3, 24, 72, count_cutoff=0).count_cutoff == 0
    assert MixedDensityEventStack(3, 24, 72, count_cutoff=127).count_cutoff == 127
    for bad in (128, -1, 10.0, "10", True):
        with pytest.raises(ValueError, match="0 .. 127"):
            MixedDensityEventStack(3, 24, 72, count_cutoff=bad)
    with pytest.raises(ValueError):
        MixedDensityEventStack(0, 24, 72)
    ef = EventFrames(720, 1280, bins=20, duration_us=50000, downsample_by_2=True, representation="mixed_density")
    assert ef.get_shape() == (20, 360, 640) and ef.count_cutoff == 10 and ef.frame_dtype == torch.int8
    assert EventFrames(720, 1280, duration_us=50000).get_shape() == (20, 720, 1280)           # the default is the stacked histogram
    assert EventFrames(720, 1280, duration_us=50000, representation="stacked_histogram").frame_dtype == torch.uint8
    es = EventStreams(3, 24, 72, bins=5, count_cutoff=None, num_events=10, representation="mixed_density")
    assert es.get_shape() == (5, 24, 72) and es.count_cutoff is None
    for cls, args in ((EventFrames, (24, 72)), (EventStreams, (3, 24, 72))):
        with pytest.raises(ValueError, match="representation"):
            cls(*args, duration_us=1000, representation="voxel_grid")
        with pytest.raises(ValueError, match="fastmode"):
            cls(*args, duration_us=1000, fastmode=False, representation="mixed_density")
        with pytest.raises(ValueError, match="0 .. 127"):
            cls(*args, duration_us=1000, count_cutoff=255, representation="mixed_density")
        with pytest.raises(ValueError, match="exactly one"):
            cls(*args, representation="mixed_density")


def test_mixed_density_call_validation():
    from sast_amd.events import EventStreams, MixedDensityEventStack
    x = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MixedDensityEventStack(10, 24, 72).construct(x, x, x, x)
    es = EventStreams(3, 24, 72, bins=20, duration_us=1000, representation="mixed_density")
    ev = torch.zeros(3, 16, dtype=torch.int64)
    counts = torch.zeros(3, dtype=torch.int64)
    ends = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError, match="t must be one of"):
        es(ev, ev, ev, ev.to(torch.int16), counts, ends)
    with pytest.raises(ValueError, match="unsupported frame geometry"):
        EventStreams(3, 24, 72, bins=513, duration_us=1000, representation="mixed_density")(ev, ev, ev, ev, counts, ends)


def test_restatement_equals_every_fixture_frame():
    """the numpy rule (bin from the fp32 exponent) against the frames the reference produced"""
    F = _fixtures()
    seen = set()
    for name, kind, bins, cut in M.CONSTRUCT:
        x, y, p, t = M.inputs(kind)
        got = M.restatement(x, y, p, t, bins, M.H, M.W, cut)
        assert got.dtype == np.int8 and np.array_equal(got, F[f"construct/{name}"]), name
        seen.add(f"construct/{name}")
    for name, kw, ends in M.BATCHED:
        x, y, p, t = M.batched_inputs(kw, ends)
        frames, bounds = M.restated_frames(x, y, p, t, kw, ends)
        assert np.array_equal(frames, F[f"batched/{name}/frames"]) and np.array_equal(bounds, F[f"batched/{name}/bounds"]), name
        seen |= {f"batched/{name}/frames", f"batched/{name}/bounds"}
    name, skw, kw, ends, _split = M.CARRY
    frames, bounds = M.restated_frames(*G.stream(**skw), kw, ends)
    assert np.array_equal(frames, F[f"batched/{name}/frames"]) and np.array_equal(bounds, F[f"batched/{name}/bounds"])
    seen |= {f"batched/{name}/frames", f"batched/{name}/bounds"}
    for s, (a, b) in enumerate(zip(M.S_FIRST, M.S_SECOND)):
        carry = 0 if M.S_RESET[s] else int(G.correct_time(G.stream(**a)[3]).max())
        frames, bounds = M.restated_frames(*G.stream(**b), M.S_KW, [row[s] for row in M.S_ENDS], t_carry=carry)
        assert np.array_equal(frames, F["streams/frames"][:, s]) and np.array_equal(bounds, F["streams/bounds"][:, s]), s
    seen |= {"streams/frames", "streams/bounds", "streams/t_last"}
    assert seen == set(F.files)


def test_fixture_cases_cover_what_they_claim():
    """the hot pixels wrap int8 and the clamp / the tie times decide bins, in the inputs the fixtures were made from"""
    x, y, p, t = M.inputs("span_50000")
    net = [int((2 * p[(x == hx) & (y == hy)] - 1).sum()) for hx, hy, _pm, _pol in M.HOT]
    assert net[0] > 255 and 127 < net[1] <= 255 and net[2] < -128 and net[3] == 0
    assert int(((x == M.BALANCED[0]) & (y == M.BALANCED[1])).sum()) > 100
    assert int(t[-1] - t[0]) == 50000
    assert M.exponent_bins(t, 24)[0] == 4 and M.exponent_bins(t, 20)[0] == 0 and M.exponent_bins(t, 24)[-1] == 23     # the 1e-6 clamp decides
    F = _fixtures()
    assert int(F["construct/span_50000_b20_cNone"][-1, 3, 5]) == ((net[0] + 128) % 256) - 128 != net[0]
    assert not F["construct/span_50000_b20_c0"].any() and F["construct/span_50000_b20_c10"].any()
    t = M.inputs("ties_2p20")[3]
    assert int(t[-1] - t[0]) == 1 << 20
    for k in range(1, 17):
        m = t == (1 << 20) >> k
        assert int(m.sum()) >= 3 and (M.exponent_bins(t, 24)[m] == 24 - k).all()
    assert int(np.ptp(M.inputs("span_7")[3])) == 7 and int(np.ptp(M.inputs("two_events_same_time")[3])) == 0
    for name, kw, ends in M.BATCHED:
        xb, yb, _p, _t = M.batched_inputs(kw, ends)
        s, e = F[f"batched/{name}/bounds"][M.EVEN_WINDOW]
        assert xb[s] % 2 == 0 and yb[s] % 2 == 0 and xb[e - 1] % 2 == 0 and yb[e - 1] % 2 == 0
        b = F[f"batched/{name}/bounds"]
        assert (b[1:, 0] < b[:-1, 1]).any()                                      # overlapping windows


def test_tool_aten_restatement_equals_fixture_frames():
    """tools/event_frames_bench.py checks the frames it times against this ATen form"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import event_frames_bench as T
    F = _fixtures()
    for name, kind, bins, cut in M.CONSTRUCT:
        x, y, p, t = (torch.from_numpy(a) for a in M.inputs(kind))
        assert np.array_equal(T.aten_md_construct(x, y, p, t, bins, M.H, M.W, cut).numpy(), F[f"construct/{name}"]), name
    name, kw, ends = M.BATCHED[0]
    x, y, p, t = (torch.from_numpy(a) for a in M.batched_inputs(kw, ends))
    got = T.aten_frames(x, y, p, t, torch.tensor(ends), kw["bins"], M.H, M.W, kw["count_cutoff"], True, kw["duration_us"], False, mixed_density=True)
    assert np.array_equal(got.numpy(), F[f"batched/{name}/frames"])


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_mixed_density_fixtures():
    """runs the reference, and with it the generator's own assertion that the reference's bin of every fixture event equals the
    exponent rule"""
    got = M.generate()
    want = _fixtures()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _i64(a):
    return torch.tensor(np.asarray(a, np.int64)).cuda()


@gpu
@pytest.mark.parametrize("name", [c[0] for c in M.CONSTRUCT])
def test_construct_matches_reference_fixture(name):
    from sast_amd.events import EventFrames, MixedDensityEventStack
    _n, kind, bins, cut = next(c for c in M.CONSTRUCT if c[0] == name)
    x, y, p, t = M.inputs(kind)
    want = torch.from_numpy(_fixtures()[f"construct/{name}"])
    rep = MixedDensityEventStack(bins, M.H, M.W, count_cutoff=cut)
    got = rep.construct(_dev(x), _dev(y), _dev(p), _dev(t))
    assert got.dtype == torch.int8 and tuple(got.shape) == rep.get_shape() == (bins, M.H, M.W)
    assert torch.equal(got.cpu(), want)
    # two calls on the same events give identical bytes
    assert torch.equal(rep.construct(_dev(x), _dev(y), _dev(p), _dev(t)), got)
    # the batched API on one count window spanning the whole stream gives the same frame
    ef = EventFrames(M.H, M.W, bins=bins, count_cutoff=cut, num_events=max(len(x), 1), representation="mixed_density")
    one = ef(_dev(x), _dev(y), _dev(p), _dev(t), _i64([int(t[-1]) if len(t) else 0]), check=True)
    assert one.dtype == torch.int8 and torch.equal(one[0].cpu(), want)


@gpu
@pytest.mark.parametrize("dxy,dt", [(torch.int16, torch.int32), (torch.int32, torch.int64), (torch.int64, torch.int32)])
def test_construct_column_dtypes(dxy, dt):
    from sast_amd.events import MixedDensityEventStack
    F = _fixtures()
    for name in ("span_50000_b20_cNone", "ties_2p20_b24", "span_7_b10"):
        _n, kind, bins, cut = next(c for c in M.CONSTRUCT if c[0] == name)
        x, y, p, t = M.inputs(kind)
        got = MixedDensityEventStack(bins, M.H, M.W, count_cutoff=cut).construct(_dev(x, dxy), _dev(y, dxy), _dev(p, dxy), _dev(t, dt))
        assert torch.equal(got.cpu(), torch.from_numpy(F[f"construct/{name}"])), name


@gpu
@pytest.mark.parametrize("name", [c[0] for c in M.BATCHED])
def test_event_frames_mixed_density_match_reference_fixture(name):
    """B = 4 overlapping windows; the first and last event of window 1 lie on even coordinates, so with downsample_by_2 t0 / t1 must
    come from the slice, not from the kept events"""
    from sast_amd.events import EventFrames, MixedDensityEventStack
    F = _fixtures()
    _n, kw, ends = next(c for c in M.BATCHED if c[0] == name)
    x, y, p, t = M.batched_inputs(kw, ends)
    ef = EventFrames(representation="mixed_density", **kw)
    out = ef(_dev(x), _dev(y), _dev(p), _dev(t), _i64(ends), check=True)
    assert out.dtype == torch.int8 and tuple(out.shape) == (4,) + ef.get_shape() == F[f"batched/{name}/frames"].shape
    assert np.array_equal(ef.last_bounds.cpu().numpy(), F[f"batched/{name}/bounds"])
    assert np.array_equal(out.cpu().numpy(), F[f"batched/{name}/frames"])
    assert ef.errors() == (0, 0)
    # B separate construct calls on the corrected slices (full resolution, then the nearest-exact rule)
    tc = G.correct_time(t)
    rep = MixedDensityEventStack(kw["bins"], M.H, M.W, count_cutoff=kw["count_cutoff"])
    for b, (s, e) in enumerate(F[f"batched/{name}/bounds"]):
        one = rep.construct(_dev(x[s:e]), _dev(y[s:e]), _dev(p[s:e]), _dev(tc[s:e]))
        if kw["downsample_by_2"]:
            one = one[:, 1::2, 1::2]
        assert torch.equal(out[b], one), b
    # the same events again, as a new recording: identical bytes
    ef.reset()
    assert torch.equal(ef(_dev(x), _dev(y), _dev(p), _dev(t), _i64(ends), check=True), out)


@gpu
def test_event_frames_mixed_density_time_carry_across_two_calls():
    from sast_amd.events import EventFrames
    F = _fixtures()
    name, skw, kw, ends, split = M.CARRY
    x, y, p, t = G.stream(**skw)
    ef = EventFrames(representation="mixed_density", **kw)
    ef(_dev(x[:split]), _dev(y[:split]), _dev(p[:split]), _dev(t[:split]), _i64(ends[:1]))      # only advances the carry
    out = ef(_dev(x[split:]), _dev(y[split:]), _dev(p[split:]), _dev(t[split:]), _i64(ends), check=True)
    assert np.array_equal(out.cpu().numpy(), F[f"batched/{name}/frames"])
    assert np.array_equal(ef.last_bounds.cpu().numpy() + split, F[f"batched/{name}/bounds"])
    assert int(ef.t_last) == int(G.correct_time(t).max())
    # without the carry the second chunk's first timestamps stay below it and the frames differ
    fresh = EventFrames(representation="mixed_density", **kw)(_dev(x[split:]), _dev(y[split:]), _dev(p[split:]), _dev(t[split:]), _i64(ends))
    assert not torch.equal(fresh, out)


@gpu
def test_mixed_density_invalid_events_and_window_capacity():
    from sast_amd.events import EventFrames, MixedDensityEventStack
    n = 3000
    x, y, p, t = G.stream(seed=9, n=n, height=M.H, width=M.W, t_step=3)
    rep = MixedDensityEventStack(10, M.H, M.W, count_cutoff=10)
    want = rep.construct(_dev(x), _dev(y), _dev(p), _dev(t))
    bx, by, bp = x.copy(), y.copy(), p.copy()
    bad = np.arange(7, n, 300)                              # 10 invalid events: x, y out of range, p = 2
    bx[bad[:4]] = M.W
    by[bad[4:7]] = -1
    bp[bad[7:]] = 2
    keep = np.ones(n, bool)
    keep[bad] = False
    assert keep[0] and keep[-1]
    with pytest.raises(ValueError, match="10 invalid events"):
        rep.construct(_dev(bx), _dev(by), _dev(bp), _dev(t))
    got = rep.construct(_dev(bx), _dev(by), _dev(bp), _dev(t), check=False)
    ref = torch.from_numpy(M.restatement(x[keep], y[keep], p[keep], t[keep], 10, M.H, M.W, 10)).cuda()
    assert torch.equal(got, ref) and not torch.equal(got, want)
    kw = dict(bins=10, count_cutoff=10, num_events=n, correct_time=False, representation="mixed_density")
    ef = EventFrames(M.H, M.W, **kw)
    f2 = ef(_dev(bx), _dev(by), _dev(bp), _dev(t), _i64([int(t[-1]), int(t[-1])]))      # two windows hold them: still counted once
    assert ef.errors() == (10, 0)
    assert torch.equal(f2[0], ref) and torch.equal(f2[1], ref)
    with pytest.raises(ValueError, match="invalid events"):
        ef(_dev(bx), _dev(by), _dev(bp), _dev(t), _i64([int(t[-1])]), check=True)
    # a window over its capacity is left zero and counted; the other window of the call is not disturbed
    ef2 = EventFrames(M.H, M.W, window_capacity=1000, **kw)
    ends2 = _i64([int(t[900]), int(t[-1])])
    f3 = ef2(_dev(x), _dev(y), _dev(p), _dev(t), ends2)
    assert ef2.errors() == (0, 1)
    e0 = int(np.searchsorted(t, t[900], side="right"))
    assert e0 <= 1000 and not f3[1].any()
    assert torch.equal(f3[0], torch.from_numpy(M.restatement(x[:e0], y[:e0], p[:e0], t[:e0], 10, M.H, M.W, 10)).cuda())
    with pytest.raises(ValueError, match="window_capacity"):
        ef2(_dev(x), _dev(y), _dev(p), _dev(t), ends2, check=True)
    # negative polarities: clipped to 0 by the reader (EventFrames), invalid for construct (the reference asserts)
    np_ = p.copy()
    np_[p == 0] = -1
    f4 = EventFrames(M.H, M.W, **kw)(_dev(x), _dev(y), _dev(np_), _dev(t), _i64([int(t[-1])]), check=True)
    assert torch.equal(f4[0], want)
    with pytest.raises(ValueError, match="invalid events"):
        rep.construct(_dev(x), _dev(y), _dev(np_), _dev(t))


_GARBAGE = (5, 5, 1, 123)      # x, y, p, t past every row's count: a valid odd pixel inside the windows


def _buffers(rows, cap, dxy=torch.int64, dt=torch.int64):
    cols = [np.full((len(rows), cap), g, np.int64) for g in _GARBAGE]
    for s, row in enumerate(rows):
        for c, a in zip(cols, row):
            c[s, :len(a)] = a
    dev = [torch.from_numpy(c).to(d).cuda() for c, d in zip(cols, (dxy, dxy, dxy, dt))]
    return dev, torch.tensor([len(r[0]) for r in rows], dtype=torch.int64).cuda()


@gpu
def test_event_streams_mixed_density_match_reference_fixture_and_separate_calls():
    """S = 3, T = 2, stale valid-looking events past every row's count; the second call resets row 1 on the device"""
    from sast_amd import _lib
    from sast_amd.events import EventFrames, EventStreams
    F = _fixtures()
    first = [G.stream(**k) for k in M.S_FIRST]
    second = [G.stream(**k) for k in M.S_SECOND]
    ends = _i64(M.S_ENDS)
    es = EventStreams(3, representation="mixed_density", **M.S_KW)
    cols, counts = _buffers(first, M.S_CAP)
    es(*cols, counts, ends)
    assert es.t_last.cpu().tolist() == [int(G.correct_time(r[3]).max()) for r in first]
    cols, counts = _buffers(second, M.S_CAP, torch.int16, torch.int32)
    rst = torch.tensor(M.S_RESET, dtype=torch.uint8).cuda()
    mine = torch.full((2, 3) + es.get_shape(), 77, dtype=torch.int8, device="cuda")
    with pytest.raises(ValueError, match="out must be a contiguous int8"):
        es(*cols, counts, ends, out=mine.to(torch.uint8))
    with pytest.raises(ValueError, match="out must be a contiguous int8"):
        es(*cols, counts, ends, out=mine[:, :, :10].contiguous())
    before = _lib.lib().sast_launch_count()
    out = es(*cols, counts, ends, reset=rst, out=mine)
    assert _lib.lib().sast_launch_count() - before == LAUNCHES_PER_CALL
    assert out is mine and out.dtype == torch.int8 and tuple(out.shape) == F["streams/frames"].shape
    assert np.array_equal(out.cpu().numpy(), F["streams/frames"])
    want_bounds = F["streams/bounds"] + (np.arange(3, dtype=np.int64) * M.S_CAP)[None, :, None]
    assert np.array_equal(es.last_bounds.cpu().numpy(), want_bounds.reshape(-1, 2))
    assert es.t_last.cpu().tolist() == F["streams/t_last"].tolist()
    assert es.errors() == (0, 0)
    # the stacked-histogram call on the same buffers takes the same number of launches
    hs = EventStreams(3, **dict(M.S_KW, bins=10))
    hs(*cols, counts, ends)
    before = _lib.lib().sast_launch_count()
    hs(*cols, counts, ends)
    assert _lib.lib().sast_launch_count() - before == LAUNCHES_PER_CALL
    # S separate EventFrames objects, each taken through the same two calls
    for s in range(3):
        ef = EventFrames(representation="mixed_density", **M.S_KW)
        a = first[s]
        ef(_dev(a[0]), _dev(a[1]), _dev(a[2]), _dev(a[3]), ends[:, s].contiguous())
        if M.S_RESET[s]:
            ef.reset()
        want = ef(*(c[s] for c in cols), ends[:, s].contiguous(), n=counts[s:s + 1], check=True)
        assert torch.equal(out[:, s], want), s
        assert int(es.t_last[s]) == int(ef.t_last)


def _signed_frames(B, H, W, seed):
    """int8 [B, 20, H, W]: sparse values in -128 .. 127, plus one 4 x 4 cell of only {-1, 0} and one of only negatives per sample"""
    g = np.random.default_rng(seed)
    x = g.integers(-128, 128, (B, 20, H, W)).astype(np.int8)
    x[g.random((B, 20, H, W)) < 0.9] = 0
    for b in range(B):
        x[b, :, 8:16, 8:24] = 0
        x[b, 3, 8:12, 8:12] = -(g.random((4, 4)) < 0.5).astype(np.int8)        # only {-1, 0}: the maximum is 0, the cell is empty
        x[b, 3, 8, 8] = -1
        x[b, 5, 12:16, 16:20] = g.integers(-128, 0, (4, 4)).astype(np.int8)    # only negatives: the maximum is non-zero
        x[b, 7, -32:, -32:] = 0                                                # a 32 x 32 cell that stays empty
    return torch.from_numpy(x).cuda()


@gpu
@pytest.mark.parametrize("shape,pad", [((2, 20, 32, 64), None), ((2, 20, 28, 60), (32, 64)), ((2, 20, 28, 92), (32, 96))])
def test_int8_frames_into_the_input_kernels_equal_the_float_copy(shape, pad):
    """input_prep (the fused kernel for the first two cases, its two-launch form for the third, whose padded size is an odd number of 32 x 32 tiles), non_zero_ratio and the NCHW -> NHWC
    copy read int8 directly and give, bit for bit, what they give for x.float()"""
    from sast_amd import functional as SF
    B, _c, H, W = shape
    x = _signed_frames(B, H, W, seed=H)
    xf = x.float()
    r8, y8 = SF.input_prep(x, pad)
    rf, yf = SF.input_prep(xf, pad)
    assert y8.dtype == torch.float32 and tuple(y8.shape) == (B,) + (tuple(pad) if pad else (H, W)) + (20,)
    assert torch.equal(r8, rf) and torch.equal(y8, yf)
    assert torch.equal(y8[:, :H, :W], xf.permute(0, 2, 3, 1)) and not y8[:, H:].any() and not y8[:, :, W:].any()
    if hasattr(yf, "sast_nonexact"):
        assert hasattr(y8, "sast_nonexact") and int(y8.sast_nonexact) == int(yf.sast_nonexact) == 0      # |v| <= 128: one bf16 each
    assert torch.equal(SF.non_zero_ratio(x, pad), SF.non_zero_ratio(xf, pad))
    assert torch.equal(SF.non_zero_ratio(x, pad), r8)
    assert torch.equal(SF.nchw_to_nhwc_float(x, pad), yf)
    # max-pool semantics on signed data: the {-1, 0} cell of channel 3 is empty, the all-negative cell of channel 5 is occupied
    Hp, Wp = pad if pad else (H, W)
    cells = (Hp // 4) * (Wp // 4)
    pooled = torch.nn.functional.max_pool2d(xf, 4)
    assert pooled[:, 3, 2, 2].eq(0).all() and pooled[:, 5, 3, 4].lt(0).all()
    want = (pooled != 0).sum((2, 3))                                            # occupied 4 x 4 cells per (sample, channel)
    assert torch.equal(r8[:, 0], np.float32(B / (B * 20 * cells)) * want.float())      # sast_rnn.py:56, B / numel * count in fp32
    anyz = (torch.nn.functional.max_pool2d(xf.abs(), 4) != 0).sum((2, 3))
    assert (want[:, 3] < anyz[:, 3]).all()                                       # "any non-zero" would count the {-1, 0} cell


@gpu
def test_mixed_density_front_end_and_backbone_in_one_graph():
    """EventFrames(bins=20, mixed density) + the backbone forward captured once after an eager warm-up, replayed on two event sets
    written into the same buffers == eager; the int8 frames reach the detector without an ATen cast"""
    from sast_amd.events import EventFrames
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_events import _detector
    net = _detector((128, 160)).eval()
    cap = 30000
    bufs = [torch.zeros(cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    ends = torch.zeros(2, dtype=torch.int64, device="cuda")
    ef = EventFrames(128, 160, bins=20, count_cutoff=10, duration_us=10000, representation="mixed_density")

    def load(seed, count):
        cols = G.stream(seed=seed, n=count, height=128, width=160, t_step=2, jitter=8)
        for buf, a in zip(bufs, cols):
            buf[:count].copy_(torch.from_numpy(a))
        n.fill_(count)
        ends.copy_(torch.tensor([10000, int(cols[3].max())]))

    def step():
        fr = ef(*bufs, ends, n=n)
        out, _st, _p = net(fr)
        return fr, out

    def flat(out):
        return [v for v in (out.values() if isinstance(out, dict) else out)]

    eager = []
    for seed, count in ((41, 30000), (42, 17000)):
        load(seed, count)
        ef.reset()
        with torch.no_grad():
            fr, out = step()
        eager.append((fr.clone(), [v.clone() for v in flat(out)]))
    assert eager[0][0].dtype == torch.int8 and tuple(eager[0][0].shape) == (2, 20, 128, 160)
    assert int(eager[0][0].lt(0).sum()) > 0 and int(eager[0][0].gt(0).sum()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    # the eager frames are the rule's, and the detector on them equals the detector on their float copy
    cols = G.stream(seed=42, n=17000, height=128, width=160, t_step=2, jitter=8)
    want, _b = M.restated_frames(*cols, dict(bins=20, height=128, width=160, count_cutoff=10, duration_us=10000), [10000, int(cols[3].max())])
    assert np.array_equal(eager[1][0].cpu().numpy(), want)
    with torch.no_grad():
        of, _st, _p = net(eager[1][0].float())
    for u, v in zip(flat(of), eager[1][1]):
        assert torch.equal(u, v)
    load(41, 30000)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            ef.reset()
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        g_fr, g_out = step()
    for (seed, count), (fr, outs) in zip(((41, 30000), (42, 17000)), eager):
        load(seed, count)
        ef.reset()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_fr, fr)
        for u, v in zip(flat(g_out), outs):
            assert torch.equal(u, v)
    assert ef.errors() == (0, 0)
