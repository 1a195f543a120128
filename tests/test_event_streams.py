"""The batched event front end: frames for S recordings side by side in one call (sast_amd.events.EventStreams, the sast_evstreams_*
entry points of csrc/k_events.hip).

GPU tests hold it to equality with what the reference gives for every recording on its own (tests/golden/event_streams.npz, written by
tests/golden/make_golden_event_streams.py; the events are regenerated from that module's integer hash) and with S separate EventFrames
calls.  Frames are compared byte for byte, bounds, carries and corrected timestamps exactly: there is no tolerance.  Every row of every
buffer carries stale, valid-looking events past its count, so reading past a count or into a neighbouring row changes a frame."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden_events as G  # noqa: E402
import make_golden_event_streams as GS  # noqa: E402

gpu = pytest.mark.gpu

LAUNCHES_PER_CALL = 7      # 2 time correction + 1 window search + 4 histogram, whatever S and T are (EventStreams' docstring)


def _fixtures():
    return np.load(os.path.join(GOLDEN, "event_streams.npz"))


def _ref_available():
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "data", "utils", "representations.py"))


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_stream_entry_points_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evstreams_")]
    assert sorted(names) == ["sast_evstreams_correct_time", "sast_evstreams_window_bounds", "sast_evstreams_ws_count"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    # the workspace query is host-only: one carry and one partial maximum per scan block, per row
    assert lib.sast_evstreams_ws_count(1) == _lib.EVENT_SCAN_BLOCKS + 1
    assert lib.sast_evstreams_ws_count(8) == 8 * (_lib.EVENT_SCAN_BLOCKS + 1)
    assert lib.sast_evstreams_ws_count(0) == 0 and lib.sast_evstreams_ws_count(65536) == 0


def test_event_streams_constructor_validation():
    from sast_amd.events import EventStreams
    with pytest.raises(ValueError, match="exactly one"):
        EventStreams(4, 720, 1280)
    with pytest.raises(ValueError, match="exactly one"):
        EventStreams(4, 720, 1280, duration_us=50000, num_events=100)
    with pytest.raises(ValueError):
        EventStreams(4, 720, 1280, num_events=0)
    with pytest.raises(ValueError, match="num_streams"):
        EventStreams(0, 720, 1280, duration_us=50000)
    with pytest.raises(ValueError):
        EventStreams(4, 720, 1280, bins=0, duration_us=50000)
    es = EventStreams(4, 720, 1280, duration_us=50000, downsample_by_2=True)
    assert es.get_shape() == (20, 360, 640) and es.num_streams == 4
    assert es.errors() == (0, 0) and es.t_last is None
    es.reset()
    es.reset(streams=[1])


def test_event_streams_call_validation():
    from sast_amd.events import EventStreams
    es = EventStreams(3, 48, 80, duration_us=1000)
    ev = torch.zeros(3, 16, dtype=torch.int64)
    counts = torch.zeros(3, dtype=torch.int64)
    ends = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_streams=3"):
        es(ev[:2], ev[:2], ev[:2], ev[:2], counts, ends)               # S != num_streams
    with pytest.raises(ValueError, match="num_streams=3"):
        es(ev[0], ev[0], ev[0], ev[0], counts, ends)                   # 1-D columns
    with pytest.raises(ValueError, match="same shape"):
        es(ev, ev, ev, ev[:, :8].contiguous(), counts, ends)
    with pytest.raises(ValueError, match="contiguous"):
        es(ev, ev, ev.t().contiguous().t(), ev, counts, ends)
    with pytest.raises(TypeError, match="x must be one of"):
        es(ev.float(), ev, ev, ev, counts, ends)
    with pytest.raises(TypeError, match="t must be one of"):
        es(ev, ev, ev, ev.to(torch.int16), counts, ends)
    with pytest.raises(ValueError, match="counts"):
        es(ev, ev, ev, ev, counts.int(), ends)
    with pytest.raises(ValueError, match="counts"):
        es(ev, ev, ev, ev, counts[:2], ends)
    with pytest.raises(ValueError, match="ends_us"):
        es(ev, ev, ev, ev, counts, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="ends_us"):
        es(ev, ev, ev, ev, counts, ends.int())
    with pytest.raises(ValueError, match="ends_us"):
        es(ev, ev, ev, ev, counts, torch.zeros(0, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="reset"):
        es(ev, ev, ev, ev, counts, ends, reset=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="reset"):
        es(ev, ev, ev, ev, counts, ends, reset=torch.zeros(2, dtype=torch.bool))
    with pytest.raises(TypeError, match="correct_time=False"):
        EventStreams(3, 48, 80, duration_us=1000, correct_time=False)(ev, ev, ev, ev.int(), counts, ends)
    # T * S beyond the windows one histogram call takes (65535)
    with pytest.raises(ValueError, match="unsupported frame geometry"):
        es(ev, ev, ev, ev, counts, torch.zeros(21846, 3, dtype=torch.int64))
    es.t_last = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="streams must be in"):
        es.reset(streams=[3])


def test_event_streams_cpu_tensors_raise_no_fallback():
    from sast_amd.events import EventStreams
    ev = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EventStreams(2, 240, 304, duration_us=50000)(ev, ev, ev, ev, torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64))


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_stream_fixtures():
    got = GS.generate()
    want = _fixtures()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------------- GPU

_GARBAGE = (5, 5, 1, 123)      # x, y, p, t past every row's count: a valid pixel (odd: it survives the downsampling) inside the windows


def _buffers(rows, cap, dxy=torch.int64, dt=torch.int64):
    """S recordings -> x, y, p, t [S, cap] and counts [S] on the device, stale events past the counts"""
    cols = [np.full((len(rows), cap), g, np.int64) for g in _GARBAGE]
    for s, row in enumerate(rows):
        for c, a in zip(cols, row):
            c[s, :len(a)] = a
    dev = [torch.from_numpy(c).to(d).cuda() for c, d in zip(cols, (dxy, dxy, dxy, dt))]
    return dev, torch.tensor([len(r[0]) for r in rows], dtype=torch.int64).cuda()


def _i64(a):
    return torch.tensor(np.asarray(a, np.int64)).cuda()


def _check_against_fixture(es, out, key, counts, cap):
    F = _fixtures()
    S = len(counts)
    assert out.dtype == torch.uint8 and tuple(out.shape) == F[f"{key}/frames"].shape
    got = out.cpu().numpy()
    for k in range(got.shape[0]):
        for s in range(S):
            assert np.array_equal(got[k, s], F[f"{key}/frames"][k, s]), (key, k, s)
    want_bounds = F[f"{key}/bounds"] + (np.arange(S, dtype=np.int64) * cap)[None, :, None]
    assert np.array_equal(es.last_bounds.cpu().numpy(), want_bounds.reshape(-1, 2))
    assert es.t_last.cpu().tolist() == F[f"{key}/t_last"].tolist()
    tc = es._state["t"].cpu().numpy().reshape(S, cap)
    for s in range(S):
        assert G.sha256(tc[s, :counts[s]]) == str(F[f"{key}/t_sha256"][s]), (key, s)
    assert es.errors() == (0, 0)


@gpu
def test_four_streams_duration_windows_match_reference_fixture():
    """case 1: rows of 5 000, 0, 1 and 777 events with jitter, T = 2; rows 2 and 3 lie below row 0's last timestamps, so a running
    maximum that crosses a row boundary changes their corrected timestamps, bounds, carries and frames"""
    from sast_amd.events import EventStreams
    rows = [G.stream(**kw) for kw in GS.ROWS]
    assert [len(r[0]) for r in rows] == [5000, 0, 1, 777] and int(rows[3][3][0]) < int(rows[0][3][-1]) > int(rows[2][3][0])
    assert any((np.diff(r[3]) < 0).any() for r in rows)                 # the time correction has work to do
    cols, counts = _buffers(rows, GS.CAP)
    es = EventStreams(4, **GS.DURATION_KW)
    out = es(*cols, counts, _i64(GS.DURATION_ENDS), check=True)
    _check_against_fixture(es, out, "duration", [5000, 0, 1, 777], GS.CAP)
    F = _fixtures()
    assert F["duration/t_last"].tolist() == [int(G.correct_time(r[3]).max()) if len(r[3]) else 0 for r in rows]
    assert F["duration/t_last"][1] == 0


@gpu
def test_count_windows_clip_at_the_start_of_their_row():
    """case 2: num_events=300 on the same rows (downsampled by 2): the rows with 1 and with ~200 events so far stop at their own first
    event, not in the tail of the row before"""
    from sast_amd.events import EventStreams
    F = _fixtures()
    assert F["count/bounds"][1, 2].tolist() == [0, 1] and F["count/bounds"][0, 3, 0] == 0 < F["count/bounds"][0, 3, 1] < 300
    cols, counts = _buffers([G.stream(**kw) for kw in GS.ROWS], GS.CAP)
    es = EventStreams(4, **GS.COUNT_KW)
    out = es(*cols, counts, _i64(GS.COUNT_ENDS), check=True)
    assert tuple(out.shape[-2:]) == (24, 40)
    _check_against_fixture(es, out, "count", [5000, 0, 1, 777], GS.CAP)


@gpu
def test_carry_and_reset_across_two_calls():
    """case 3: rows 0 and 3 continue their recording (carry kept: call 2 starts with an event below it), row 1 gets nothing new, row 2
    starts a new recording with `reset` set; then the host-side reset of one row, and a device-side reset on an empty chunk"""
    from sast_amd.events import EventStreams
    first, second = GS.carry_rows()
    es = EventStreams(4, **GS.CARRY_KW)
    cols, counts = _buffers(first, GS.CAP)
    es(*cols, counts, _i64(GS.CARRY_ENDS))
    assert es.t_last.cpu().tolist() == [int(G.correct_time(r[3]).max()) for r in first]
    cols, counts = _buffers(second, GS.CAP)
    out = es(*cols, counts, _i64(GS.CARRY_ENDS), reset=torch.tensor(GS.CARRY_RESET, dtype=torch.uint8).cuda(), check=True)
    _check_against_fixture(es, out, "carry", [len(r[0]) for r in second], GS.CAP)
    want = _fixtures()["carry/t_last"].tolist()
    es.reset(streams=[0])
    assert es.t_last.cpu().tolist() == [0] + want[1:]
    # a row that starts a new recording with an empty chunk: the reset still takes effect, the other carries stay
    es(*cols, torch.zeros(4, dtype=torch.int64).cuda(), _i64(GS.CARRY_ENDS), reset=torch.tensor([False, False, False, True]).cuda())
    assert es.t_last.cpu().tolist() == [0, want[1], want[2], 0]
    es.reset()
    assert es.t_last.cpu().tolist() == [0, 0, 0, 0]


@gpu
@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("dxy,dt", [(torch.int16, torch.int32), (torch.int64, torch.int64)])
def test_streams_equal_separate_event_frames_calls(dxy, dt, ds):
    """case 4: one call == S EventFrames calls on the rows; ends_us [S] == ends_us [1, S][0]"""
    from sast_amd.events import EventFrames, EventStreams
    kw = dict(GS.DURATION_KW, downsample_by_2=ds)
    rows = [G.stream(**k) for k in GS.ROWS]
    cols, counts = _buffers(rows, GS.CAP, dxy, dt)
    ends = _i64(GS.DURATION_ENDS)
    es = EventStreams(4, **kw)
    out = es(*cols, counts, ends, check=True)
    for s in range(4):
        ef = EventFrames(**kw)
        want = ef(*(c[s] for c in cols), ends[:, s].contiguous(), n=counts[s:s + 1], check=True)
        assert torch.equal(out[:, s], want), s
        assert torch.equal(es.last_bounds.view(2, 4, 2)[:, s] - s * GS.CAP, ef.last_bounds)
        assert int(es.t_last[s]) == int(ef.t_last)
    es.reset()
    one = es(*cols, counts, ends[1].contiguous(), check=True)
    es.reset()
    assert tuple(one.shape) == (4,) + es.get_shape()
    assert torch.equal(one, es(*cols, counts, ends[1:2].contiguous(), check=True)[0])
    assert torch.equal(one, out[1])


@gpu
def test_full_size_rows_hash_to_the_committed_reference_frames():
    """case 5: the gen1_carry recording of events.npz in rows 0 and 2 of three Gen1-sized rows, another recording between them"""
    from sast_amd.events import EventFrames, EventStreams
    _n, kw, fkw, ends, _split = next(c for c in G.BATCHED if c[0] == "gen1_carry")
    rec = G.stream(**kw)
    other = G.stream(seed=24, n=90000, height=240, width=304, t_start=30000, t_step=3, jitter=200)
    cap = len(rec[0])
    cols, counts = _buffers([rec, other, rec], cap)
    ends_ts = _i64([[e] * 3 for e in ends])
    es = EventStreams(3, **fkw)
    out = es(*cols, counts, ends_ts, check=True)
    want = str(np.load(os.path.join(GOLDEN, "events.npz"))["batched/gen1_carry/sha256"])
    assert G.sha256(out[:, 0].cpu().numpy()) == want
    assert G.sha256(out[:, 2].cpu().numpy()) == want
    mid = EventFrames(**fkw)(*(c[1] for c in cols), _i64(ends), n=counts[1:2], check=True)
    assert torch.equal(out[:, 1], mid) and int(mid.count_nonzero()) > 0


@gpu
def test_invalid_events_in_one_row_are_skipped_and_counted_once():
    """case 6"""
    from sast_amd.events import EventStreams
    rows = [G.stream(seed=50 + s, n=2000, height=GS.H, width=GS.W, t_step=3) for s in range(3)]
    x, y, p, t = (a.copy() for a in rows[1])
    bad = np.arange(7, 2000, 200)                          # 10 invalid events: x, y out of range, p = 2
    x[bad[:4]] = GS.W
    y[bad[4:7]] = -1
    p[bad[7:]] = 2
    keep = np.ones(2000, bool)
    keep[bad] = False
    assert keep[0] and keep[-1]
    ends = _i64([[int(r[3][-1]) for r in rows]] * 2)       # two windows holding the same events: still counted once
    kw = dict(height=GS.H, width=GS.W, bins=10, count_cutoff=10, num_events=2000, correct_time=False)
    cols, counts = _buffers(rows, 2500)
    clean = EventStreams(3, **kw)(*cols, counts, ends, check=True)
    with pytest.raises(ValueError, match="6 windows hold more events than window_capacity"):      # left empty and reported
        EventStreams(3, window_capacity=100, **kw)(*cols, counts, ends, check=True)
    cols, counts = _buffers([rows[0], tuple(a[keep] for a in rows[1]), rows[2]], 2500)
    kept = EventStreams(3, **kw)(*cols, counts, ends, check=True)     # skipped, not written: the frame of the valid events
    cols, counts = _buffers([rows[0], (x, y, p, t), rows[2]], 2500)
    es = EventStreams(3, **kw)
    out = es(*cols, counts, ends)
    assert es.errors() == (10, 0)
    assert torch.equal(out[:, 0], clean[:, 0]) and torch.equal(out[:, 2], clean[:, 2])
    assert torch.equal(out[:, 1], kept[:, 1]) and not torch.equal(out[:, 1], clean[:, 1])
    assert es.t_last.cpu().tolist() == [0, 0, 0]           # correct_time=False leaves the carries alone
    with pytest.raises(ValueError, match="10 invalid events"):
        es(*cols, counts, ends, check=True)


@gpu
def test_launch_count_does_not_grow_with_the_number_of_streams():
    """case 7"""
    from sast_amd import _lib
    from sast_amd.events import EventStreams
    lib = _lib.lib()
    for S in (1, 8):
        rows = [G.stream(seed=60 + s, n=500 + 100 * s, height=GS.H, width=GS.W, t_step=3, jitter=10) for s in range(S)]
        cols, counts = _buffers(rows, 1500)
        es = EventStreams(S, **GS.DURATION_KW)
        for T in (1, 3):
            ends = _i64([[1000 * (k + 1)] * S for k in range(T)])
            es(*cols, counts, ends)                         # warm-up: workspaces
            before = lib.sast_launch_count()
            es(*cols, counts, ends)
            assert lib.sast_launch_count() - before == LAUNCHES_PER_CALL, (S, T)
    torch.cuda.synchronize()


@gpu
def test_event_streams_and_backbone_in_one_graph():
    """case 8: EventStreams (S = 2) + the backbone forward captured once, replayed on new events, counts, ends and a reset flag written
    into the same tensors == the same two steps run eagerly"""
    from sast_amd.events import EventStreams
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_events import _detector
    net = _detector((128, 160)).eval()
    S, cap = 2, 20000
    bufs = [torch.zeros(S, cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    counts = torch.zeros(S, dtype=torch.int64, device="cuda")
    ends = torch.zeros(S, dtype=torch.int64, device="cuda")
    rst = torch.zeros(S, dtype=torch.uint8, device="cuda")
    es = EventStreams(S, 128, 160, bins=10, count_cutoff=10, duration_us=10000)
    # step 1: two recordings start; step 2: row 0 starts a new recording (reset), row 1 continues below its carry
    steps = [(((41, 20000, 0), (42, 9000, 500)), (0, 0)), (((43, 12000, 0), (44, 15000, 0)), (1, 0))]

    def load(step):
        recs, flags = step
        for s, (seed, n, t_start) in enumerate(recs):
            cols = G.stream(seed=seed, n=n, height=128, width=160, t_start=t_start, t_step=2, jitter=8)
            for buf, a in zip(bufs, cols):
                buf[s, :n].copy_(torch.from_numpy(a))
            counts[s] = n
            ends[s] = int(cols[3].max()) - 100 * s
        rst.copy_(torch.tensor(flags, dtype=torch.uint8))

    def step():
        fr = es(*bufs, counts, ends, reset=rst)
        out, _st, _p = net(fr)
        return fr, out

    def flat(out):
        return [v for v in (out.values() if isinstance(out, dict) else out)]

    eager = []
    with torch.no_grad():
        for st in steps:
            load(st)
            fr, out = step()
            eager.append((fr.clone(), es.t_last.clone(), [v.clone() for v in flat(out)]))
    assert int(eager[1][0][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    es.reset()
    load(steps[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        g_fr, g_out = step()
    es.reset()
    for st, (fr, t_last, outs) in zip(steps, eager):
        load(st)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_fr, fr)
        assert torch.equal(es.t_last, t_last)
        for u, v in zip(flat(g_out), outs):
            assert torch.equal(u, v)
    assert es.errors() == (0, 0)
