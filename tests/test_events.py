"""Raw events -> stacked-histogram frames (sast_amd/events.py, csrc/k_events.hip).

GPU tests hold the device front end to bit equality with frames the reference produced (tests/golden/events.npz, written by
tests/golden/make_golden_events.py); the event streams are regenerated from that module's integer hash, so nothing here reads the
reference on the GPU box.  CPU tests: argument checks (the ABI of the struct: tests/test_abi.py), and -- where the reference is present -- that the
generator reproduces every committed fixture and that the timing tool's ATen restatement of construct equals the reference's."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_events as G  # noqa: E402

gpu = pytest.mark.gpu


def _fixtures():
    return np.load(os.path.join(GOLDEN, "events.npz"))


def _ref_available():
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "data", "utils", "representations.py"))


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_event_entry_points_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_event_")]
    assert sorted(names) == ["sast_event_correct_time", "sast_event_frames", "sast_event_frames_ws_bytes", "sast_event_window_bounds"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    # the workspace query is host-only: geometry limits
    assert lib.sast_event_frames_ws_bytes(4, 10, 720, 1280, 1, 1 << 20) > 4 * (1 << 22)
    assert lib.sast_event_frames_ws_bytes(1, 321, 240, 304, 0, 16) == 0       # 2 * bins > 640
    assert lib.sast_event_frames_ws_bytes(0, 10, 240, 304, 0, 16) == 0


def test_events_cpu_tensors_raise_no_fallback():
    from sast_amd.events import EventFrames, StackedHistogram
    x = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StackedHistogram(10, 240, 304).construct(x, x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EventFrames(240, 304, duration_us=50000)(x, x, x, x, torch.zeros(1, dtype=torch.int64))


def test_events_argument_validation():
    from sast_amd.events import EventFrames, StackedHistogram
    with pytest.raises(ValueError):
        StackedHistogram(0, 240, 304)
    with pytest.raises(ValueError):
        StackedHistogram(10, 240, 304, count_cutoff=0)
    assert StackedHistogram(10, 240, 304, count_cutoff=1000).count_cutoff == 255
    assert StackedHistogram(10, 240, 304).count_cutoff == 255
    assert StackedHistogram(3, 240, 304).get_shape() == (6, 240, 304)
    with pytest.raises(ValueError, match="exactly one"):
        EventFrames(720, 1280)
    with pytest.raises(ValueError, match="exactly one"):
        EventFrames(720, 1280, duration_us=50000, num_events=100)
    with pytest.raises(ValueError):
        EventFrames(720, 1280, num_events=0)
    assert EventFrames(720, 1280, duration_us=50000, downsample_by_2=True).get_shape() == (20, 360, 640)


def test_event_stream_generator_is_plain_integer_arithmetic():
    x, y, p, t = G.stream(seed=1, n=1000, height=10, width=20, t_step=4, hot=((3, 4, 500, 1),), jitter=5)
    assert x.dtype == y.dtype == p.dtype == t.dtype == np.int64
    assert x.min() >= 0 and x.max() < 20 and y.min() >= 0 and y.max() < 10 and set(np.unique(p)) <= {0, 1}
    assert 400 < int(((x == 3) & (y == 4)).sum()) < 600
    assert (np.diff(t) < 0).any() and t.min() >= 0                     # jitter: unsorted, fixed by the time correction
    assert np.array_equal(G.stream(seed=1, n=1000, height=10, width=20)[0], G.stream(seed=1, n=1000, height=10, width=20)[0])


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_fixtures():
    got = G.generate()
    want = _fixtures()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_tool_aten_restatement_equals_reference():
    import event_frames_bench as T
    rep = G.load_representations()
    for seed, (bins, cut, fast) in enumerate([(10, 10, True), (1, None, False), (5, 255, True), (10, None, False)]):
        x, y, p, t = G.stream(seed=100 + seed, n=30000, height=24, width=40, t_step=7, hot=((3, 5, 600, 1),))
        tx, ty, tp, tt = (torch.from_numpy(a) for a in (x, y, p, t))
        want = rep.StackedHistogram(bins, 24, 40, count_cutoff=cut, fastmode=fast).construct(tx, ty, tp, tt)
        got = T.aten_construct(tx, ty, tp, tt, bins, 24, 40, 255 if cut is None else cut, fast)
        assert torch.equal(got, want), (bins, cut, fast)


# ---------------------------------------------------------------------------------------------------------------------------- GPU

_DTYPES = {"gen1_duration_i16": (torch.int16, torch.int32)}     # (x / y / p, t) of a case; int64 otherwise


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


@gpu
@pytest.mark.parametrize("name", [c[0] for c in G.CONSTRUCT])
def test_stacked_histogram_matches_reference_fixture(name):
    from sast_amd.events import StackedHistogram
    _n, kw, (bins, h, w, cut, fast) = next(c for c in G.CONSTRUCT if c[0] == name)
    x, y, p, t = G.construct_inputs(kw)
    want = torch.from_numpy(_fixtures()[f"construct/{name}"])
    rep = StackedHistogram(bins, h, w, count_cutoff=cut, fastmode=fast)
    got = rep.construct(_dev(x), _dev(y), _dev(p), _dev(t))
    assert got.dtype == torch.uint8 and tuple(got.shape) == rep.get_shape()
    assert torch.equal(got.cpu(), want)
    if name == "gen1_full":       # the sensor's native widths give the same frame
        got2 = rep.construct(_dev(x, torch.int16), _dev(y, torch.int16), _dev(p, torch.int32), _dev(t, torch.int32))
        assert torch.equal(got2.cpu(), want)


@gpu
@pytest.mark.parametrize("name", [c[0] for c in G.CONSTRUCT])
def test_event_frames_single_window_matches_construct_fixture(name):
    """the batched API on one count window spanning the whole stream equals construct (sorted streams: no time change)"""
    from sast_amd.events import EventFrames
    _n, kw, (bins, h, w, cut, fast) = next(c for c in G.CONSTRUCT if c[0] == name)
    x, y, p, t = G.construct_inputs(kw)
    want = torch.from_numpy(_fixtures()[f"construct/{name}"])
    ef = EventFrames(h, w, bins=bins, count_cutoff=cut, fastmode=fast, num_events=max(len(x), 1))
    end = int(t[-1]) if len(t) else 0
    got = ef(_dev(x), _dev(y), _dev(p), _dev(t), _dev([end]), check=True)
    assert torch.equal(got[0].cpu(), want)


def _run_batched(name, chunked=False):
    from sast_amd.events import EventFrames
    _n, kw, fkw, ends, split = next(c for c in G.BATCHED if c[0] == name)
    x, y, p, t = G.stream(**kw)
    dxy, dt = _DTYPES.get(name, (torch.int64, torch.int64))
    ef = EventFrames(**fkw)
    if split is not None and chunked:
        # chunk 1 only advances the time-correction carry; the windows lie in chunk 2
        ef(_dev(x[:split], dxy), _dev(y[:split], dxy), _dev(p[:split], dxy), _dev(t[:split], dt), _dev(ends[:1]))
        x, y, p, t = x[split:], y[split:], p[split:], t[split:]
    out = ef(_dev(x, dxy), _dev(y, dxy), _dev(p, dxy), _dev(t, dt), _dev(ends), check=True)
    return ef, out, split


@gpu
@pytest.mark.parametrize("name", [c[0] for c in G.BATCHED])
def test_event_frames_match_reference_fixture(name):
    F = _fixtures()
    ef, out, split = _run_batched(name)
    frames = out.cpu().numpy()
    assert torch.equal(torch.from_numpy(G.crops(frames)), torch.from_numpy(F[f"batched/{name}/crops"]))
    assert np.array_equal(ef.last_bounds.cpu().numpy(), F[f"batched/{name}/bounds"])
    assert [int(np.count_nonzero(f)) for f in frames] == F[f"batched/{name}/nonzero"].tolist()
    assert G.sha256(frames) == str(F[f"batched/{name}/sha256"])
    assert G.sha256(ef._state["t"][:len(G.stream(**next(c for c in G.BATCHED if c[0] == name)[1])[0])].cpu().numpy()) == \
        str(F[f"batched/{name}/t_sha256"])
    assert ef.errors() == (0, 0)


@gpu
def test_event_frames_time_carry_across_two_chunks():
    F = _fixtures()
    name = "gen1_carry"
    ef, out, split = _run_batched(name, chunked=True)
    frames = out.cpu().numpy()
    assert G.sha256(frames) == str(F[f"batched/{name}/sha256"])
    assert np.array_equal(ef.last_bounds.cpu().numpy() + split, F[f"batched/{name}/bounds"])
    # the carry is the running maximum of everything seen, and reset() starts a new recording
    t = G.correct_time(G.stream(**next(c for c in G.BATCHED if c[0] == name)[1])[3])
    assert int(ef.t_last) == int(t.max())
    ef.reset()
    assert int(ef.t_last) == 0


@gpu
def test_invalid_events_are_skipped_and_reported():
    from sast_amd.events import EventFrames, StackedHistogram
    x, y, p, t = G.stream(seed=9, n=5000, height=24, width=40, t_step=3)
    want = StackedHistogram(10, 24, 40, count_cutoff=10).construct(_dev(x), _dev(y), _dev(p), _dev(t))
    bx, by, bp = x.copy(), y.copy(), p.copy()
    bad = np.arange(7, 5000, 500)                          # 10 invalid events: x, y out of range, p = 2
    bx[bad[:4]] = 40
    by[bad[4:7]] = -1
    bp[bad[7:]] = 2
    keep = np.ones(5000, bool)
    keep[bad] = False
    rep = StackedHistogram(10, 24, 40, count_cutoff=10)
    with pytest.raises(ValueError, match="10 invalid events"):
        rep.construct(_dev(bx), _dev(by), _dev(bp), _dev(t))
    got = rep.construct(_dev(bx), _dev(by), _dev(bp), _dev(t), check=False)
    # skipped, not written: equal to the frame of the valid events over the same time span (first / last events stay valid)
    assert keep[0] and keep[-1]
    ref = rep.construct(_dev(x[keep]), _dev(y[keep]), _dev(p[keep]), _dev(t[keep]))
    assert torch.equal(got, ref)
    assert not torch.equal(got, want)
    ef = EventFrames(24, 40, bins=10, count_cutoff=10, num_events=5000, correct_time=False)
    f = ef(_dev(bx), _dev(by), _dev(bp), _dev(t), _dev([int(t[-1])]))
    torch.cuda.synchronize()
    assert ef.errors() == (10, 0)
    assert torch.equal(f[0], ref)
    # two windows holding the same events: every invalid event is still reported once
    ef.reset()
    f2 = ef(_dev(bx), _dev(by), _dev(bp), _dev(t), _dev([int(t[-1]), int(t[-1])]))
    assert ef.errors() == (10, 0)
    assert torch.equal(f2[0], ref) and torch.equal(f2[1], ref)
    with pytest.raises(ValueError, match="invalid events"):
        ef(_dev(bx), _dev(by), _dev(bp), _dev(t), _dev([int(t[-1])]), check=True)
    # a window over its capacity is left empty and reported
    ef2 = EventFrames(24, 40, bins=10, count_cutoff=10, num_events=5000, window_capacity=100)
    with pytest.raises(ValueError, match="window_capacity"):
        ef2(_dev(x), _dev(y), _dev(p), _dev(t), _dev([int(t[-1])]), check=True)
    # negative polarities: clipped to 0 by the reader (EventFrames), invalid for construct (the reference asserts)
    np_ = p.copy()
    np_[p == 0] = -1
    f3 = EventFrames(24, 40, bins=10, count_cutoff=10, num_events=5000, correct_time=False)(_dev(x), _dev(y), _dev(np_), _dev(t),
                                                                                           _dev([int(t[-1])]), check=True)
    assert torch.equal(f3[0], want)
    with pytest.raises(ValueError, match="invalid events"):
        rep.construct(_dev(x), _dev(y), _dev(np_), _dev(t))


def _detector(hw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import sast_oracle as O
    from sast_amd.detection import RNNDetector
    from test_gpu_parity import _rcfg, load_params
    ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=(4, 5), embed_dim=32, amp=2e-2)
    params = O.init_backbone_params(ocfg, seed=3, ls_init=0.5)
    net = RNNDetector(_rcfg(hw, (4, 5), 32, 2e-2, 0.5)).cuda()
    load_params(net, params)
    return net


@gpu
def test_frames_from_raw_events_feed_the_detector_like_fixture_frames():
    """a Gen1 frame made on the GPU from raw events and the reference's frame of the same events loaded from events.npz give the same
    RNNDetector outputs over two steps with the recurrent states carried"""
    from sast_amd.events import EventFrames
    net = _detector((256, 320)).eval()
    _n, kw, (bins, h, w, cut, fast) = next(c for c in G.CONSTRUCT if c[0] == "gen1_full")
    x, y, p, t = G.construct_inputs(kw)
    ef = EventFrames(h, w, bins=bins, count_cutoff=cut, fastmode=fast, num_events=len(x))
    frames = ef(_dev(x, torch.int16), _dev(y, torch.int16), _dev(p, torch.int16), _dev(t, torch.int32), _dev([int(t[-1])]), check=True)
    fixture = torch.from_numpy(_fixtures()["construct/gen1_full"]).cuda().unsqueeze(0)
    assert frames.shape == fixture.shape == (1, 20, 240, 304)
    assert torch.equal(frames, fixture)
    st_a = st_b = None
    with torch.no_grad():
        for _step in range(2):
            oa, st_a, _ = net(frames, st_a)
            ob, st_b, _ = net(fixture, st_b)
            for u, v in zip(oa.values(), ob.values()):
                assert torch.equal(u, v)
            for (ha, ca), (hb, cb) in zip(st_a, st_b):
                assert torch.equal(ha, hb) and torch.equal(ca, cb)


@gpu
def test_event_front_end_and_backbone_in_one_graph():
    """EventFrames + the backbone forward captured once, replayed on two event sets written into the same buffers == eager"""
    from sast_amd.events import EventFrames
    net = _detector((128, 160)).eval()
    cap = 30000
    bufs = [torch.zeros(cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    ends = torch.zeros(2, dtype=torch.int64, device="cuda")
    ef = EventFrames(128, 160, bins=10, count_cutoff=10, duration_us=10000)

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


@gpu
def test_time_correction_and_window_search_do_not_depend_on_the_entry_point():
    """one recording through the single-recording calls (512 scan blocks of 5 events, the last 12 with an empty chunk, and a carry loop
    that strides over more partial maxima than a block has threads from block 256 on) and through the per-row calls with S = 1 (one
    block): the same kernels on two grids give what numpy gives, and neither reads or writes past the count"""
    from sast_amd import _lib as L
    from sast_amd.functional import _stream
    lib = L.lib()
    cap, n, sentinel = 3000, 2500, -7
    t = np.full(cap, 2 ** 31 - 1, dtype=np.int64)
    t[:n] = G.stream(seed=77, n=n, height=24, width=40, t_step=4, jitter=30)[3]
    carry = int(np.sort(t[:n])[25]) + 1
    assert (t[:5] < carry).all() and (np.diff(t[:n]) < 0).any()
    want = np.maximum.accumulate(np.maximum(t[:n], carry))
    t_dev, n_dev = _dev(t, torch.int32), _dev([n])
    scan = torch.empty(int(lib.sast_evstreams_ws_count(1)), dtype=torch.int64, device="cuda")
    assert scan.numel() == L.EVENT_SCAN_BLOCKS + 1
    corrected = []
    for rows in (False, True):
        t_out = torch.full((cap,), sentinel, dtype=torch.int64, device="cuda")
        t_last = _dev([carry])
        if rows:
            L.check(lib.sast_evstreams_correct_time(t_dev.data_ptr(), L.DT_I32, n_dev.data_ptr(), 1, cap, t_out.data_ptr(),
                                                    t_last.data_ptr(), None, scan.data_ptr(), _stream()), "evstreams_correct_time")
        else:
            L.check(lib.sast_event_correct_time(t_dev.data_ptr(), L.DT_I32, n_dev.data_ptr(), cap, t_out.data_ptr(), t_last.data_ptr(),
                                                scan.data_ptr(), _stream()), "event_correct_time")
        got = t_out.cpu().numpy()
        assert np.array_equal(got[:n], want), rows
        assert int(t_last) == int(want[-1]), rows
        assert (got[n:] == sentinel).all(), rows
        corrected.append(t_out)
    repeated = int(want[np.flatnonzero(np.diff(want) == 0)[600]])
    ends = np.array([want[0] - 1, want[-1] + 5, repeated, want[300], want[1700]], dtype=np.int64)
    end = np.searchsorted(want, ends, "right")
    assert end[0] == 0 and end[1] == n and end[2] - np.searchsorted(want, repeated, "left") >= 2
    ends_dev = _dev(ends)
    for mode, value in ((L.EVENT_WINDOW_DURATION, 500), (L.EVENT_WINDOW_COUNT, 700)):
        start = np.maximum(end - value, 0) if mode == L.EVENT_WINDOW_COUNT else np.searchsorted(want, ends - value, "left")
        assert mode != L.EVENT_WINDOW_COUNT or 0 < end[3] < value                  # a count window clipped at the first event
        for rows, tc in zip((False, True), corrected):
            bounds = torch.full((5, 2), sentinel, dtype=torch.int64, device="cuda")
            if rows:
                L.check(lib.sast_evstreams_window_bounds(tc.data_ptr(), n_dev.data_ptr(), 1, cap, ends_dev.data_ptr(), 5, mode, value,
                                                         bounds.data_ptr(), _stream()), "evstreams_window_bounds")
            else:
                L.check(lib.sast_event_window_bounds(tc.data_ptr(), n_dev.data_ptr(), cap, ends_dev.data_ptr(), 5, mode, value,
                                                     bounds.data_ptr(), _stream()), "event_window_bounds")
            assert np.array_equal(bounds.cpu().numpy(), np.stack([start, end], 1)), (mode, rows)
