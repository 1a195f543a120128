"""Event retention across chunks (sast_amd.events.EventQueue, the sast_evqueue_* entry points of csrc/k_events.hip).

The queue is held to equality with one `EventStreams` call on the whole recordings (frames byte for byte, window bounds as event
identities, carries) and, step by step, with a numpy model of its state (tests/event_queue_model.py), which the CPU tests in turn hold
to whole-recording window bounds.  Everything is integers: there is no tolerance.  Every chunk row carries stale, valid-looking events
past its count, and the queue's storage is filled with such events before the first push."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import event_queue_model as M  # noqa: E402
import make_golden_dat as GD  # noqa: E402
import make_golden_event_streams as GS  # noqa: E402
import make_golden_events as G  # noqa: E402

gpu = pytest.mark.gpu

PUSH_LAUNCHES, FRAMES_LAUNCHES = 2, 7      # EventQueue's docstring: partial maxima, scan + decode + append; 1 search + 4 frames + 2 retire
_GEO = dict(height=GS.H, width=GS.W)
_MODES = {"duration": (M.DURATION, dict(duration_us=600)), "count": (M.COUNT, dict(num_events=300))}
_LENGTHS = (5000, 0, 1234, 3000)


def _rows(seed, lengths=_LENGTHS, **kw):
    return [G.stream(seed=seed + k, n=n, t_start=100 * k, t_step=4, jitter=60, **_GEO, **kw) for k, n in enumerate(lengths)]


def _ref_available():
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "utils", "evaluation", "prophesee", "io", "dat_events_tools.py"))


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_queue_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evqueue_")]
    assert sorted(names) == ["sast_evqueue_push", "sast_evqueue_retire", "sast_evqueue_window_bounds", "sast_evqueue_ws_count"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert [f for f, _t in _lib.SastEvQueueArgs._fields_] == ["x", "y", "p", "t", "head", "count", "t_last", "retired", "retired_t", "err",
                                                              "ws", "capacity", "S", "reserved"]


def test_queue_workspace_count_follows_its_formula():
    from sast_amd import _lib
    lib = _lib.lib()
    for S in (1, 8, 65535):
        assert lib.sast_evqueue_ws_count(S) == S * (_lib.EVENT_SCAN_BLOCKS + 6)
    assert lib.sast_evqueue_ws_count(0) == 0 and lib.sast_evqueue_ws_count(-3) == 0 and lib.sast_evqueue_ws_count(65536) == 0


def _fake_args(**over):
    """a SastEvQueueArgs of non-null, never dereferenced pointers: the checks run before any launch"""
    from sast_amd import _lib
    a = _lib.SastEvQueueArgs()
    for f, _t in _lib.SastEvQueueArgs._fields_[:11]:
        setattr(a, f, 0x1000)
    a.capacity, a.S = 1024, 4
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_queue_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    EINVAL = -22
    p, I64, I32, I16, DAT = 0x1000, _lib.DT_I64, _lib.DT_I32, _lib.DT_I16, _lib.EVQUEUE_DT_DAT

    def push(a, x=p, y=p, pol=p, t=p, codes=(I64, I64, I64, I64), counts=p, chunk=256):
        return lib.sast_evqueue_push(None if a is None else C.byref(a), x, y, pol, t, *codes, counts, chunk, None, None)

    bad_queues = [None] + [_fake_args(**{f: None}) for f in ("x", "y", "p", "t", "head", "count", "t_last", "retired", "retired_t", "err", "ws")]
    bad_queues += [_fake_args(S=0), _fake_args(S=65536), _fake_args(capacity=0), _fake_args(capacity=-5), _fake_args(S=4, capacity=2 ** 29)]
    for a in bad_queues:
        assert push(a) == EINVAL
        assert lib.sast_evqueue_window_bounds(None if a is None else C.byref(a), p, 1, 0, 100, p, None) == EINVAL
        assert lib.sast_evqueue_retire(None if a is None else C.byref(a), p, 1, None) == EINVAL
    a = _fake_args()
    for kw in (dict(x=None), dict(y=None), dict(pol=None), dict(t=None), dict(counts=None), dict(chunk=-1), dict(chunk=2 ** 30),
               dict(codes=(_lib.DT_F32, I64, I64, I64)), dict(codes=(I64, _lib.DT_U8, I64, I64)), dict(codes=(I64, I64, 7, I64)),
               dict(codes=(I64, I64, I64, I16)), dict(codes=(I64, I64, I64, 7)), dict(codes=(DAT, DAT, DAT, I64))):
        assert push(a, **kw) == EINVAL, kw
    assert push(a, x=None, y=None, pol=None, t=None, codes=(DAT,) * 4) == EINVAL       # packed records still need their pointer
    for kw in (dict(ends=None), dict(bounds=None), dict(T=0), dict(T=2 ** 30), dict(mode=2), dict(value=-1)):
        k = dict(ends=p, T=1, mode=0, value=100, bounds=p)
        k.update(kw)
        assert lib.sast_evqueue_window_bounds(C.byref(a), k["ends"], k["T"], k["mode"], k["value"], k["bounds"], None) == EINVAL, kw
    assert lib.sast_evqueue_retire(C.byref(a), None, 1, None) == EINVAL
    assert lib.sast_evqueue_retire(C.byref(a), p, 0, None) == EINVAL
    assert lib.sast_evqueue_retire(C.byref(a), p, 2 ** 30, None) == EINVAL


def test_event_queue_constructor_validation():
    from sast_amd.events import EventQueue
    with pytest.raises(ValueError, match="exactly one"):
        EventQueue(4, 1000, 720, 1280)
    with pytest.raises(ValueError, match="exactly one"):
        EventQueue(4, 1000, 720, 1280, duration_us=50000, num_events=100)
    with pytest.raises(ValueError):
        EventQueue(4, 1000, 720, 1280, num_events=0)
    with pytest.raises(ValueError, match="num_streams"):
        EventQueue(0, 1000, 720, 1280, duration_us=50000)
    with pytest.raises(ValueError, match="capacity"):
        EventQueue(4, 0, 720, 1280, duration_us=50000)
    with pytest.raises(ValueError, match="2\\^31"):
        EventQueue(4, 2 ** 29, 720, 1280, duration_us=50000)
    with pytest.raises(ValueError, match="32767"):
        EventQueue(4, 1000, 32768, 1280, duration_us=50000)
    with pytest.raises(ValueError, match="32767"):
        EventQueue(4, 1000, 720, 40000, duration_us=50000)
    with pytest.raises(ValueError, match="representation"):
        EventQueue(4, 1000, 720, 1280, duration_us=50000, representation="voxels")
    q = EventQueue(4, 1000, 720, 1280, duration_us=50000, downsample_by_2=True)
    assert q.get_shape() == (20, 360, 640) and q.num_streams == 4 and q.capacity == 1000
    assert EventQueue(4, 1000, 720, 1280, num_events=5, representation="mixed_density").get_shape() == (10, 720, 1280)
    assert q.errors() == (0, 0, 0, 0) and q.t_last is None
    assert (q.PUSH_LAUNCHES, q.FRAMES_LAUNCHES) == (PUSH_LAUNCHES, FRAMES_LAUNCHES)
    q.reset()
    q.reset(streams=[1])


def test_event_queue_call_validation():
    from sast_amd.events import EventQueue
    q = EventQueue(3, 64, 48, 80, duration_us=1000)
    ev = torch.zeros(3, 16, dtype=torch.int64)
    counts = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="num_streams=3"):
        q.push(ev[:2], ev[:2], ev[:2], ev[:2], counts)
    with pytest.raises(ValueError, match="num_streams=3"):
        q.push(ev[0], ev[0], ev[0], ev[0], counts)
    with pytest.raises(ValueError, match="same shape"):
        q.push(ev, ev, ev, ev[:, :8].contiguous(), counts)
    with pytest.raises(ValueError, match="contiguous"):
        q.push(ev, ev, ev.t().contiguous().t(), ev, counts)
    with pytest.raises(TypeError, match="x must be one of"):
        q.push(ev.float(), ev, ev, ev, counts)
    with pytest.raises(TypeError, match="t must be one of"):
        q.push(ev, ev, ev, ev.to(torch.int16), counts)
    with pytest.raises(ValueError, match="counts"):
        q.push(ev, ev, ev, ev, counts.int())
    with pytest.raises(ValueError, match="counts"):
        q.push(ev, ev, ev, ev, counts[:2])
    with pytest.raises(ValueError, match="reset"):
        q.push(ev, ev, ev, ev, counts, reset=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="reset"):
        q.push(ev, ev, ev, ev, counts, reset=torch.zeros(2, dtype=torch.bool))
    rec = torch.zeros(3, 16, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="records must be"):
        q.push_dat(rec[:2], counts)
    with pytest.raises(ValueError, match="records must be"):
        q.push_dat(torch.zeros(3, 16, 3, dtype=torch.int32), counts)
    with pytest.raises(ValueError, match="records must be"):
        q.push_dat(rec[:, :, 0], counts)
    with pytest.raises(TypeError, match="int32"):
        q.push_dat(rec.long(), counts)
    with pytest.raises(ValueError, match="contiguous"):
        q.push_dat(torch.zeros(3, 2, 16, dtype=torch.int32).transpose(1, 2), counts)
    with pytest.raises(ValueError, match="counts"):
        q.push_dat(rec, counts.int())
    with pytest.raises(ValueError, match="ends_us"):
        q.frames(torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="ends_us"):
        q.frames(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="ends_us"):
        q.frames(torch.zeros(0, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="ends_us"):
        q.frames(torch.zeros(3, 2, dtype=torch.int64).t())
    with pytest.raises(ValueError, match="unsupported frame geometry"):
        q.frames(torch.zeros(21846, 3, dtype=torch.int64))


def test_event_queue_cpu_tensors_raise_no_fallback():
    from sast_amd.events import EventQueue
    q = EventQueue(2, 64, 240, 304, duration_us=50000)
    ev = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.push(ev, ev, ev, ev, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.push_dat(torch.zeros(2, 4, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.frames(torch.zeros(1, 2, dtype=torch.int64))


def _model_session(model, rows, rounds):
    ident = []
    for cuts, ends in rounds:
        model.push([tuple(c[lo:hi] for c in r) for r, (lo, hi) in zip(rows, cuts)])
        ident.append(model.frames(ends)[1])
    return np.concatenate(ident), np.concatenate([e for _c, e in rounds])


@pytest.mark.parametrize("mode", ["duration", "count"])
@pytest.mark.parametrize("seed", range(6))
def test_model_reproduces_whole_recording_bounds_over_random_chunkings(mode, seed):
    """append, the retire rule and the live <= head compaction: windows found in the retained events are the whole recording's"""
    code, kw = _MODES[mode]
    value = list(kw.values())[0]
    rows = _rows(70 + 10 * seed)
    rounds = M.schedule([r[3] for r in rows], seed, 400, value)
    model = M.QueueModel(4, 1400, code, value)
    ident, ends = _model_session(model, rows, rounds)
    for s in range(4):
        assert np.array_equal(ident[:, s], M.whole_bounds(rows[s][3], ends[:, s], code, value)), s
    assert model.err.tolist() == [0, 0, 0, 0]
    assert model.moves[0] >= 3 and model.moves_skipped[0] >= 1 and model.moves[1] == 0
    assert model.t_last.tolist() == [int(G.correct_time(r[3]).max()) if len(r[3]) else 0 for r in rows]


def test_model_counts_drops_and_late_windows():
    rows = _rows(40, lengths=(2000, 2000))
    for code, value in ((M.DURATION, 600), (M.COUNT, 300)):
        model = M.QueueModel(2, 1200, code, value)
        model.push([tuple(c[:900] for c in r) for r in rows])
        model.push([tuple(c[900:1500] for c in rows[0]), tuple(c[900:1000] for c in rows[1])])
        assert model.err.tolist() == [0, 0, 300, 0] and model.count.tolist() == [1200, 1000]
        assert model.t_last[0] == G.correct_time(rows[0][3])[1199]             # the carry advances over the stored events only
        end = int(model.t[0, 1100])
        model.frames([[end, end]])
        assert model.err[3] == 0 and model.retired[0] > 0
        model.frames([[end - value - 50, end]])                                 # row 0 goes back, row 1 does not
        assert model.err.tolist() == [0, 0, 300, 1]


def test_sizing_rule_counts_every_push_between_two_frames_calls():
    """capacity >= 2 R + P: R the live events right after a `frames` call, P everything pushed before the next one.  Four chunks of a
    quarter window per call, window k asked for after the first chunk of window k + 1: R = 1.25 windows, P = 1 window -> 3.5 windows
    never drop, 3 windows (one chunk per call assumed) do"""
    E, T, D = 2000, 4, 3000
    x, y, p, _t = G.stream(seed=97, n=T * E, **_GEO)
    t = (np.arange(T * E, dtype=np.int64) * D) // E                            # E events per window of D us
    ends = [(k + 1) * D - 1 for k in range(T)]
    dropped = {}
    for cap in (3 * E, 7 * E // 2):
        model, ident = M.QueueModel(1, cap, M.DURATION, D - 1), []
        for i in range(4 * T):
            model.push([tuple(c[i * E // 4:(i + 1) * E // 4] for c in (x, y, p, t))])
            for k in ([i // 4 - 1] if i and i % 4 == 0 else []) + ([T - 1] if i == 4 * T - 1 else []):
                ident.append(model.frames([[ends[k]]])[1][0, 0])
        dropped[cap] = int(model.err[2])
        if not dropped[cap]:
            assert np.array_equal(np.stack(ident), M.whole_bounds(t, ends, M.DURATION, D - 1))
            assert np.array_equal(np.stack(ident), [[k * E, (k + 1) * E] for k in range(T)])
    assert dropped == {3 * E: E // 4, 7 * E // 2: 0}


def test_packed_records_decode_to_the_committed_reference_columns():
    F = np.load(os.path.join(GOLDEN, "dat_events.npz"))
    rec = F["records"]
    assert rec.dtype == np.int32 and rec.shape == (GD.N, 2) and np.array_equal(rec, GD.records())
    x, y, p, t = M.decode_dat(rec)
    for got, key in ((x, "x"), (y, "y"), (p, "p"), (t, "t")):
        assert np.array_equal(got, F[key].astype(np.int64)), key
    w1 = rec.view(np.uint32)[:, 1]
    assert (w1 >> 29).max() == 7 and (t >= 2 ** 31).sum() > 50 and (t < 2 ** 31).sum() > 50      # bits 29-31 set; the unsigned clock
    assert x.max() == 16383 and y.max() == 16383 and set(p.tolist()) == {0, 1}
    assert np.array_equal(M.encode_dat(x, y, p, t, w1 >> 29), rec)
    assert os.path.getsize(os.path.join(GOLDEN, "dat_events.npz")) < 100 * 1024


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_dat_fixture():
    got = GD.generate()
    want = np.load(os.path.join(GOLDEN, "dat_events.npz"))
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------------- GPU

_GARBAGE = (5, 5, 1, 123)      # x, y, p, t past every chunk row's count and all over the fresh storage: a valid pixel that survives downsampling


def _i64(a):
    return torch.tensor(np.asarray(a, np.int64)).cuda()


def _chunk(parts, chunk_cap, dxy=torch.int64, dt=torch.int64):
    """S chunk rows -> x, y, p, t [S, chunk_cap] and counts [S] on the device, stale events past the counts"""
    cols = [np.full((len(parts), chunk_cap), g, np.int64) for g in _GARBAGE]
    for s, part in enumerate(parts):
        for c, a in zip(cols, part):
            c[s, :len(a)] = a
    return [torch.from_numpy(c).to(d).cuda() for c, d in zip(cols, (dxy, dxy, dxy, dt))], _i64([len(part[0]) for part in parts])


def _queue(S, capacity, **kw):
    from sast_amd.events import EventQueue
    q = EventQueue(S, capacity, **kw)
    q._storage(torch.device("cuda", torch.cuda.current_device()))
    for col, g in zip((q.x, q.y, q.p, q.t), _GARBAGE):
        col.fill_(g)
    return q


def _state_equals_model(q, model, rows=None):
    for name in ("head", "count", "t_last", "retired", "retired_t"):
        assert getattr(q, name).cpu().tolist() == getattr(model, name).tolist(), name
    for s in (range(q.num_streams) if rows is None else rows):
        h, c = int(model.head[s]), int(model.count[s])
        for name in ("x", "y", "p", "t"):
            assert np.array_equal(getattr(q, name)[s, h:c].cpu().numpy(), getattr(model, name)[s, h:c]), (name, s)


def _session(q, model, rows, rounds, chunk_cap, resets=None, dxy=torch.int64, dt=torch.int64, push=None):
    """push / frames round by round on the device and in the model, state compared after every call -> (frames [sum T, S, ...], event
    identities of the bounds [sum T, S, 2])"""
    frames, ident = [], []
    S, cap = q.num_streams, q.capacity
    for r, (cuts, ends) in enumerate(rounds):
        parts = [tuple(c[lo:hi] for c in row) for row, (lo, hi) in zip(rows, cuts)]
        rst = None if resets is None or resets[r] is None else resets[r]
        cols, counts = _chunk(parts, chunk_cap, dxy, dt)
        args = () if rst is None else (torch.tensor(rst, dtype=torch.uint8).cuda(),)
        if push is not None:
            push(q, parts, counts, *args)
        else:
            q.push(*cols, counts, *args)
        model.push(parts, rst)
        _state_equals_model(q, model)
        origin = model.origin.copy()
        fr = q.frames(_i64(ends))
        b, i = model.frames(ends)
        got = q.last_bounds.cpu().numpy().reshape(-1, S, 2) - (np.arange(S, dtype=np.int64) * cap)[None, :, None]
        assert np.array_equal(got, b), r
        assert np.array_equal(got + origin[None, :, None], i)
        _state_equals_model(q, model)
        frames.append(fr)
        ident.append(i)
    return torch.cat(frames), np.concatenate(ident)


def _whole(rows, ends, cap=None, check=True, **kw):
    """one EventStreams call on the whole recordings -> (frames [T, S, ...], bounds [T, S, 2] row-relative, t_last)"""
    from sast_amd.events import EventStreams
    S = len(rows)
    cap = cap or max(max(len(r[0]) for r in rows), 1)
    cols, counts = _chunk(rows, cap)
    es = EventStreams(S, **kw)
    out = es(*cols, counts, _i64(ends), check=check)
    b = es.last_bounds.cpu().numpy().reshape(-1, S, 2) - (np.arange(S, dtype=np.int64) * cap)[None, :, None]
    return out, b, es.t_last.cpu().tolist()


# pushes of the pinned case, events per row: a 0-event chunk, a 1-event chunk, cuts inside the first windows; `frames` after the
# fourth and after the last push
_PINNED_PUSHES = [(0, 0, 0, 0), (1, 0, 1, 1), (699, 0, 0, 299), (1800, 0, 0, 0), (100, 0, 0, 477), (2400, 0, 0, 0)]
_PINNED_FRAMES_AFTER = (3, 5)


def _pinned_rounds(ends):
    done = np.zeros(4, np.int64)
    rounds, step = [], 0
    for k, n in enumerate(_PINNED_PUSHES):
        cuts = np.stack([done, done + np.asarray(n)], 1)
        done = cuts[:, 1].copy()
        rounds.append((cuts, np.asarray(ends[step], np.int64)[None] if k in _PINNED_FRAMES_AFTER else None))
        step += k in _PINNED_FRAMES_AFTER
    return rounds


def _pinned_run(kw, ends):
    """-> frames [2, 4, ...] and the queue"""
    rows = [G.stream(**k) for k in GS.ROWS]
    q = _queue(4, GS.CAP, **kw)
    out = []
    for cuts, e in _pinned_rounds(ends):
        cols, counts = _chunk([tuple(c[lo:hi] for c in row) for row, (lo, hi) in zip(rows, cuts)], 2400)
        q.push(*cols, counts)
        if e is not None:
            out.append(q.frames(_i64(e), check=True)[0])
    assert q.count.cpu().tolist()[1] == 0 and int(q.retired.sum()) > 0
    return torch.stack(out), q, rows


@gpu
@pytest.mark.parametrize("key", ["duration", "count"])
def test_chunked_rows_match_the_reference_fixture_step_by_step(key):
    """case 1: the four rows of event_streams.npz pushed in six chunks, one `frames` call per step"""
    kw, ends = (GS.DURATION_KW, GS.DURATION_ENDS) if key == "duration" else (GS.COUNT_KW, GS.COUNT_ENDS)
    F = np.load(os.path.join(GOLDEN, "event_streams.npz"))
    out, q, _rows_ = _pinned_run(kw, ends)
    got = out.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == F[f"{key}/frames"].shape
    for k in range(2):
        for s in range(4):
            assert np.array_equal(got[k, s], F[f"{key}/frames"][k, s]), (k, s)
    assert q.t_last.cpu().tolist() == F[f"{key}/t_last"].tolist()
    assert q.errors() == (0, 0, 0, 0)


@gpu
def test_chunked_rows_match_event_streams_in_mixed_density():
    """case 1, representation="mixed_density": against one EventStreams call on the whole rows"""
    kw = dict(GS.DURATION_KW, representation="mixed_density")
    out, q, rows = _pinned_run(kw, GS.DURATION_ENDS)
    want, _b, t_last = _whole(rows, GS.DURATION_ENDS, GS.CAP, **kw)
    assert out.dtype == torch.int8 and torch.equal(out, want) and int(out.count_nonzero()) > 0
    assert q.t_last.cpu().tolist() == t_last


@gpu
@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("rep", ["stacked_histogram", "mixed_density"])
@pytest.mark.parametrize("mode", ["duration", "count"])
@pytest.mark.parametrize("seed", [0, 3])
def test_random_chunkings_equal_the_whole_recording(seed, mode, rep, ds):
    """case 2: S = 4 rows of 5 000, 0, 1 234 and 3 000 events in chunks of 0 .. 400, T = 1 .. 3 steps per call, capacity 1 400: rows are
    compacted several times and a compaction is skipped (live > head) as well"""
    code, wkw = _MODES[mode]
    value = list(wkw.values())[0]
    kw = dict(bins=10, count_cutoff=10, downsample_by_2=ds, representation=rep, **_GEO, **wkw)
    rows = _rows(70 + 10 * seed)
    rounds = M.schedule([r[3] for r in rows], seed, 400, value)
    q, model = _queue(4, 1400, **kw), M.QueueModel(4, 1400, code, value)
    frames, ident = _session(q, model, rows, rounds, 400)
    assert model.moves[0] >= 3 and model.moves_skipped[0] >= 1             # both happened (the device's head / count followed the model)
    ends = np.concatenate([e for _c, e in rounds])
    want, bounds, t_last = _whole(rows, ends, **kw)
    assert torch.equal(frames, want) and int(frames.count_nonzero()) > 0
    assert np.array_equal(ident, bounds)
    assert q.t_last.cpu().tolist() == t_last
    assert q.errors() == (0, 0, 0, 0)


def _row_rounds(t, seed, value, T=2):
    return M.schedule([t], seed, 300, value, steps=(T,))


def _zip_rounds(per_row, T=2):
    """rounds of single rows side by side; a row whose session is over pushes nothing and repeats its last end"""
    n = max(len(r) for r in per_row)
    out = []
    for k in range(n):
        cuts, ends = [], []
        for r in per_row:
            c, e = r[min(k, len(r) - 1)]
            cuts.append(c[0] if k < len(r) else (c[0, 1], c[0, 1]))
            ends.append(e[:, 0] if k < len(r) else np.full(T, e[-1, 0]))
        out.append((np.asarray(cuts, np.int64), np.stack(ends, 1)))
    return out


@gpu
@pytest.mark.parametrize("mode", ["duration", "count"])
def test_reset_of_one_row_mid_stream(mode):
    """case 3: row 1 starts a new recording at round 3, its old clock (50 000 us and up) far above the new one's"""
    code, wkw = _MODES[mode]
    value = list(wkw.values())[0]
    kw = dict(bins=10, count_cutoff=10, **_GEO, **wkw)
    r0, r2 = _rows(20, lengths=(2500, 1800))
    old = G.stream(seed=27, n=900, t_start=50000, t_step=4, jitter=60, **_GEO)
    new = G.stream(seed=28, n=1500, t_start=0, t_step=4, jitter=60, **_GEO)
    K = 3
    s0, s2 = _row_rounds(r0[3], 1, value), _row_rounds(r2[3], 2, value)
    s_old, s_new = _row_rounds(old[3], 3, value)[:K], _row_rounds(new[3], 4, value)
    assert s_old[-1][0][0, 1] > 400 and s_old[-1][1][-1, 0] > 50000 > 10 * s_new[-1][1][-1, 0]
    # row 1's events: the pushed part of the old recording, then the new one (the new rounds' cuts shifted behind it)
    n_old = int(s_old[-1][0][0, 1])
    row1 = tuple(np.concatenate([a[:n_old], b]) for a, b in zip(old, new))
    s1 = s_old + [(c + n_old, e) for c, e in s_new]
    rounds = _zip_rounds([s0, s1, s2])
    resets = [None] * K + [[0, 1, 0]] + [None] * (len(rounds) - K - 1)
    rows = [r0, row1, r2]
    ma = M.QueueModel(3, 1400, code, value)
    fa = _session(_queue(3, 1400, **kw), ma, rows, rounds, 300, resets)[0]
    assert ma.err.tolist() == [0, 0, 0, 0]                                    # the row's ends went back, but the row was reset first
    # without the reset: the other rows do not notice
    qb = _queue(3, 1400, **kw)
    fb = _session(qb, M.QueueModel(3, 1400, code, value), rows, rounds, 300)[0]
    assert torch.equal(fa[:, 0], fb[:, 0]) and torch.equal(fa[:, 2], fb[:, 2]) and not torch.equal(fa[:, 1], fb[:, 1])
    # a fresh queue fed only the new recording
    none = np.zeros((1, 2), np.int64), np.zeros((2, 1), np.int64)
    fresh = _zip_rounds([[none], s_new, [none]])
    qc, mc = _queue(3, 1400, **kw), M.QueueModel(3, 1400, code, value)
    fc = _session(qc, mc, [r0, new, r2], fresh, 300)[0]
    n = 2 * len(s_new)
    assert torch.equal(fa[2 * K:2 * K + n, 1], fc[:n, 1]) and int(fc[:, 1].count_nonzero()) > 0
    assert int(mc.t_last[1]) == int(G.correct_time(new[3]).max()) == int(ma.t_last[1])
    assert [int(v[1]) for v in (ma.head, ma.count, ma.retired, ma.retired_t)] == [int(v[1]) for v in (mc.head, mc.count, mc.retired, mc.retired_t)]


@gpu
def test_overflowing_row_drops_counts_and_stays_inside_its_storage():
    """case 4: row 1 is pushed 1 500 events with room for 1 200, then goes on after its first windows; row 2 behind it is a canary"""
    kw = dict(bins=10, count_cutoff=10, duration_us=600, **_GEO)
    rows = _rows(50, lengths=(1100, 2200, 0))
    pushes = [(300, 500, 0), (300, 500, 0), (300, 500, 0), (200, 700, 0)]
    done = np.zeros(3, np.int64)
    rounds = []
    for k, n in enumerate(pushes):
        cuts = np.stack([done, done + np.asarray(n)], 1)
        done = cuts[:, 1].copy()
        rounds.append(cuts)
    tc = [G.correct_time(r[3]) for r in rows[:2]]

    def run(capacity):
        q, model = _queue(3, capacity, **kw), M.QueueModel(3, capacity, M.DURATION, 600)
        canary = [c[2].clone() for c in (q.x, q.y, q.p, q.t)]
        out = []
        for k, cuts in enumerate(rounds):
            parts = [tuple(c[lo:hi] for c in row) for row, (lo, hi) in zip(rows, cuts)]
            cols, counts = _chunk(parts, 700)
            q.push(*cols, counts)
            model.push(parts)
            _state_equals_model(q, model)
            if k >= 2:
                ends = [[int(tc[0][cuts[0, 1] - 1]) - 1, int(model.t_last[1]) - 1, 0]]
                out.append(q.frames(_i64(ends)))
                model.frames(ends)
                _state_equals_model(q, model)
        for c, want in zip((q.x, q.y, q.p, q.t), canary):
            assert torch.equal(c[2], want)
        return torch.cat(out), q, model

    big, qb, mb = run(4000)
    assert qb.errors() == (0, 0, 0, 0)
    small, q, model = run(1200)
    assert model.err[2] == 300 and q.errors() == (0, 0, 300, 0)                   # the third push: 200 of its 500 events fit
    assert torch.equal(small[:, 0], big[:, 0]) and not torch.equal(small[:, 1], big[:, 1])
    with pytest.raises(ValueError, match=f"{int(model.err[2])} events were dropped"):
        q.frames(_i64([[10 ** 6] * 3]), check=True)
    assert q.errors() == (0, 0, 0, 0)


@gpu
@pytest.mark.parametrize("mode", ["duration", "count"])
def test_window_that_goes_back_after_retirement_is_counted_late(mode):
    """case 5"""
    code, wkw = _MODES[mode]
    value = list(wkw.values())[0]
    rows = _rows(40, lengths=(2000, 2000))
    q, model = _queue(2, 2400, bins=10, count_cutoff=10, **_GEO, **wkw), M.QueueModel(2, 2400, code, value)
    cols, counts = _chunk(rows, 2000)
    q.push(*cols, counts)
    model.push(rows)
    end = int(model.t[0, 1500])
    for ends in ([[end - 40, end - 40], [end, end]], [[end, end]]):           # monotone, a repeated end included
        q.frames(_i64(ends))
        model.frames(ends)
    assert q.errors() == (0, 0, 0, 0) and int(q.retired[0]) > 0
    q.frames(_i64([[end - value - 50, end]]))                                   # row 0 goes back, row 1 does not
    model.frames([[end - value - 50, end]])
    assert model.err.tolist() == [0, 0, 0, 1] and q.errors() == (0, 0, 0, 1)
    _state_equals_model(q, model)
    with pytest.raises(ValueError, match="1 late windows"):
        q.frames(_i64([[end, end]]), check=True)


def _dat_rows():
    """row 0: the fixture's records (clock around 2^31, events off the sensor among them); row 1: a recording packed by the model"""
    F = np.load(os.path.join(GOLDEN, "dat_events.npz"))
    x, y, p, t = G.stream(seed=95, n=1500, t_start=300, t_step=4, jitter=60, **_GEO)
    rec1 = M.encode_dat(x, y, p, t, high_bits=np.arange(1500) % 8)
    return [F["records"], rec1], [tuple(F[k].astype(np.int64) for k in "xypt"), (x, y, p, t)]


@gpu
@pytest.mark.parametrize("ds", [False, True])
def test_packed_records_equal_decoded_columns(ds):
    """case 6: push_dat of the fixture records == push of the columns the reference's reader returns for them"""
    recs, rows = _dat_rows()
    kw = dict(bins=10, count_cutoff=10, duration_us=600, downsample_by_2=ds, **_GEO)
    rounds = M.schedule([r[3] for r in rows], 5, 400, 600)
    assert rows[0][3].max() >= 2 ** 31 and (rows[0][0] >= GS.W).any()

    def push_dat(q, parts, counts, *rst):
        buf = np.tile(np.asarray([[_GARBAGE[3], _GARBAGE[0] | _GARBAGE[1] << 14 | _GARBAGE[2] << 28]], np.int32), (2, 400, 1))
        for s, part in enumerate(parts):
            buf[s, :len(part[0])] = M.encode_dat(*part, high_bits=(np.arange(len(part[0])) + s) % 8)
        q.push_dat(torch.from_numpy(buf).cuda(), counts, *rst)

    for s in range(2):                                                          # the packing helper agrees with the stored records
        assert np.array_equal(M.decode_dat(recs[s]), np.stack(rows[s]))
    qa, ma = _queue(2, 1400, **kw), M.QueueModel(2, 1400, M.DURATION, 600)
    fa, ia = _session(qa, ma, rows, rounds, 400)
    qb, mb = _queue(2, 1400, **kw), M.QueueModel(2, 1400, M.DURATION, 600)
    fb, ib = _session(qb, mb, rows, rounds, 400, push=push_dat)
    assert torch.equal(fa, fb) and np.array_equal(ia, ib) and int(fa[:, 0].count_nonzero()) > 0
    assert qa.t_last.cpu().tolist() == qb.t_last.cpu().tolist() == [int(G.correct_time(r[3]).max()) for r in rows]
    assert qa.errors() == qb.errors() and qa.errors()[0] > 0 and qa.errors()[1:] == (0, 0, 0)
    want, bounds, _t = _whole(rows, np.concatenate([e for _c, e in rounds]), check=False, **kw)
    assert torch.equal(fa, want) and np.array_equal(ia, bounds)


@gpu
def test_column_dtypes_agree_and_narrowing_saturates():
    """case 6: int16 / int32 / int64 chunks give the same queue; x = 65541 and p = 65537 are invalid events, not pixel 5 / polarity 1"""
    kw = dict(bins=10, count_cutoff=10, duration_us=600, **_GEO)
    rows = _rows(60, lengths=(1500, 700))
    rounds = M.schedule([r[3] for r in rows], 6, 400, 600)
    runs = []
    for dxy, dt in ((torch.int16, torch.int32), (torch.int32, torch.int32), (torch.int64, torch.int64)):
        q = _queue(2, 1400, **kw)
        runs.append((_session(q, M.QueueModel(2, 1400, M.DURATION, 600), rows, rounds, 400, dxy=dxy, dt=dt)[0], q))
    for f, q in runs[1:]:
        assert torch.equal(f, runs[0][0]) and q.errors() == (0, 0, 0, 0)
    x, y, p, t = (a.copy() for a in rows[0])
    bad = np.arange(7, 1500, 150)                                               # 10 events
    x[bad[:4]] = 65541
    y[bad[4:6]] = -65531                                                        # wraps to 5 without saturation
    p[bad[6:]] = 65537
    keep = np.ones(1500, bool)
    keep[bad] = False
    end = [[int(G.correct_time(t).max()), 10 ** 6]]
    wkw = dict(kw, duration_us=10 ** 6)
    for dxy in (torch.int32, torch.int64):
        q = _queue(2, 1600, **wkw)
        q.push(*_chunk([(x, y, p, t), rows[1]], 1500, dxy=dxy)[0], _i64([1500, 700]))
        assert int(q.x[0, 7]) == 32767 and int(q.y[0, bad[4]]) == -32768 and int(q.p[0, bad[6]]) == 32767
        got = q.frames(_i64(end))
        assert q.errors() == (10, 0, 0, 0)
        qk = _queue(2, 1600, **wkw)
        qk.push(*_chunk([tuple(a[keep] for a in rows[0]), rows[1]], 1500)[0], _i64([1490, 700]))
        assert torch.equal(got, qk.frames(_i64(end), check=True))


@gpu
def test_queue_launch_counts_are_the_documented_ones():
    """case 7"""
    from sast_amd import _lib
    lib = _lib.lib()
    for S in (1, 8):
        rows = [G.stream(seed=60 + s, n=1500, t_step=3, jitter=10, **_GEO) for s in range(S)]
        q = _queue(S, 4000, **GS.DURATION_KW)
        done = 0
        for chunk in (100, 600):
            cols, counts = _chunk([tuple(c[done:done + chunk] for c in r) for r in rows], chunk)
            rec = torch.zeros(S, chunk, 2, dtype=torch.int32).cuda()
            done += chunk
            for T in (1, 3):
                ends = _i64([[1000 * (k + 1)] * S for k in range(T)])
                q.frames(ends)                                  # warm-up: workspaces
                before = lib.sast_launch_count()
                q.push(*cols, counts)
                assert lib.sast_launch_count() - before == PUSH_LAUNCHES, (S, T, chunk)
                before = lib.sast_launch_count()
                q.push_dat(rec, torch.zeros_like(counts))
                assert lib.sast_launch_count() - before == PUSH_LAUNCHES, (S, T, chunk)
                before = lib.sast_launch_count()
                q.frames(ends)
                assert lib.sast_launch_count() - before == FRAMES_LAUNCHES, (S, T, chunk)
    torch.cuda.synchronize()


@gpu
def test_push_and_frames_in_one_graph():
    """case 8: push + frames captured once after a warm-up, replayed on three new chunks (counts, ends and a reset flag written into the
    same tensors) == the eager run"""
    S, chunk_cap = 2, 500
    kw = dict(bins=10, count_cutoff=10, duration_us=600, **_GEO)
    rows = _rows(80, lengths=(1200, 900))
    other = G.stream(seed=88, n=400, t_start=0, t_step=4, jitter=60, **_GEO)
    # (row 0 part, row 1 part), reset flags, ends [2, S]: at the third step row 0 starts a new recording
    # (every chunk spans more than the 200 us between a call's two ends, so a row's ends never go back)
    steps = [((rows[0], 0, 500), (rows[1], 0, 300), (0, 0)), ((rows[0], 500, 1000), (rows[1], 300, 600), (0, 0)),
             ((other, 0, 400), (rows[1], 600, 900), (1, 0))]
    bufs = [torch.zeros(S, chunk_cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    counts = torch.zeros(S, dtype=torch.int64, device="cuda")
    ends = torch.zeros(2, S, dtype=torch.int64, device="cuda")
    rst = torch.zeros(S, dtype=torch.uint8, device="cuda")

    def load(step):
        e = []
        for s, (rec, lo, hi) in enumerate(step[:2]):
            for buf, a, g in zip(bufs, rec, _GARBAGE):
                buf[s].fill_(g)
                buf[s, :hi - lo].copy_(torch.from_numpy(a[lo:hi]))
            counts[s] = hi - lo
            top = int(G.correct_time(rec[3])[hi - 1]) - 1
            e.append((top - 200, top))
        ends.copy_(torch.tensor(e, dtype=torch.int64).t())
        rst.copy_(torch.tensor(step[2], dtype=torch.uint8))

    def call(q):
        q.push(*bufs, counts, reset=rst)
        return q.frames(ends)

    qe, model = _queue(S, 1400, **kw), M.QueueModel(S, 1400, M.DURATION, 600)
    eager = []
    for st in steps:
        load(st)
        fr = call(qe)
        model.push([tuple(c[lo:hi] for c in rec) for rec, lo, hi in st[:2]], st[2])
        model.frames(ends.cpu().numpy())
        _state_equals_model(qe, model)
        eager.append((fr.clone(), [v.clone() for v in (qe.head, qe.count, qe.t_last, qe.retired, qe.retired_t)]))
    assert int(eager[2][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0]) and qe.errors() == (0, 0, 0, 0)
    q = _queue(S, 1400, **kw)
    load(steps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(q)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_fr = call(q)
    q.reset()
    for st, (fr, state) in zip(steps, eager):
        load(st)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_fr, fr)
        for u, v in zip((q.head, q.count, q.t_last, q.retired, q.retired_t), state):
            assert torch.equal(u, v)
    assert q.errors() == (0, 0, 0, 0)
