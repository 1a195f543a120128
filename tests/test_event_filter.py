"""sast_amd.events.EventFilter on the MI355X (csrc/k_evfilter.hip) against the sequential model of tests/event_filter_model.py: the kept
events x, y, p, t, n, the surface, t_last, seen, kept and the counter, EQUAL, no tolerance (everything is integers).  Every chunk row
carries stale events past its count that would change the answer, and every randomised test first asserts on the MODEL that between
0.10 and 0.90 of the events pass: an expected answer of "all" or "none" proves nothing."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import event_filter_model as M  # noqa: E402
import event_queue_model as QM  # noqa: E402
import test_online_detector as TO  # noqa: E402
from test_online_detector import detector  # noqa: E402,F401  (the tiny detector of the online tests, a module-scoped fixture)

gpu = pytest.mark.gpu

SENSORS = [(5, 7), (12, 16), (48, 64)]
COUNTS_1 = (0, 1, 63, 64, 65, 257, 5000)                        # S = 1: one recording in consecutive chunks of these sizes
COUNTS_3 = ((5000, 0, 257), (65, 1, 0), (0, 63, 64))            # S = 3: consecutive calls, different counts per row, one row empty
_GARBAGE = (1, 1, 1, 2 ** 40)                                   # past every row's count: a pixel inside every sensor, a time far ahead
DT = {torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}


def _i64(a):
    return torch.tensor(np.asarray(a, np.int64)).cuda()


def _u8(a):
    return torch.tensor(np.asarray(a, np.uint8)).cuda()


def _chunk(parts, cap, dxy=torch.int64, dt=torch.int64):
    cols = [np.full((len(parts), cap), g, np.int64) for g in _GARBAGE]
    for s, part in enumerate(parts):
        for c, a in zip(cols, part):
            c[s, :len(a)] = a
    if dt == torch.int32:
        cols[3] = np.minimum(cols[3], 2 ** 31 - 1)
    return [torch.from_numpy(c.astype(DT[d])).cuda() for c, d in zip(cols, (dxy, dxy, dxy, dt))], _i64([len(p[0]) for p in parts])


def _filter(S, hw, mode, threshold_us=None, radius=1):
    from sast_amd.events import EventFilter
    thr = M.thresholds(*hw)[mode] if threshold_us is None else threshold_us
    return (EventFilter(S, hw[0], hw[1], mode=mode, threshold_us=thr, radius=radius),
            [M.FilterModel(hw[0], hw[1], mode, thr, radius) for _ in range(S)])


def _in_band(kept, seen):
    assert 0.10 <= kept / max(seen, 1) <= 0.90, (kept, seen)


def _out_equals(out, want):
    """the filter's five tensors against per-row (x, y, p, t) of the model"""
    x, y, p, t, n = (v.cpu().numpy() for v in out)
    assert (x.dtype, y.dtype, p.dtype, t.dtype, n.dtype) == (np.int16, np.int16, np.int16, np.int64, np.int64)
    assert n.tolist() == [len(w[0]) for w in want]
    for s, w in enumerate(want):
        for name, got, exp in zip("xypt", (x, y, p, t), w):
            assert np.array_equal(got[s, :n[s]], exp), (name, s)


def _state_equals(f, models):
    assert np.array_equal(f.surface.cpu().numpy(), np.stack([m.surface for m in models]))
    assert f.t_last.cpu().tolist() == [m.t_last for m in models]
    assert f.seen.cpu().tolist() == [m.seen for m in models] and f.kept.cpu().tolist() == [m.kept for m in models]
    assert f.errors() == (sum(m.err for m in models),)


def _call(f, models, parts, cap, reset=None, **kw):
    """one device call and the model's pushes of the same parts -> the model's rows; outputs and state compared"""
    cols, counts = _chunk(parts, cap, **kw)
    out = f(*cols, counts, None if reset is None else _u8(reset))
    want = [m.push(*part, reset=bool(reset is not None and reset[s]))[:4] for s, (m, part) in enumerate(zip(models, parts))]
    _out_equals(out, want)
    _state_equals(f, models)
    return want


def _consecutive(recs, sizes):
    """per call the parts of the rows: row s of call k takes the next sizes[k][s] events of recs[s]"""
    at, calls = [0] * len(recs), []
    for size in sizes:
        calls.append([tuple(c[at[s]:at[s] + size[s]] for c in recs[s]) for s in range(len(recs))])
        at = [a + n for a, n in zip(at, size)]
    return calls


def _model_rate(recs, hw, mode, **kw):
    out, models = M.run(recs, hw[0], hw[1], mode=mode, threshold_us=kw.pop("threshold_us", M.thresholds(*hw)[mode]), **kw)
    _in_band(sum(m.kept for m in models), sum(m.seen for m in models))
    return out, models


@gpu
@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("hw", SENSORS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("S", [1, 3])
def test_filter_equals_the_model_over_counts_and_streams(S, hw, mode):
    sizes = [(n,) for n in COUNTS_1] if S == 1 else COUNTS_3
    recs = [M.recording(10 * S + s, sum(z[s] for z in sizes), *hw) for s in range(S)]
    assert all(r[3].min() > 2 ** 33 for r in recs) and any((r[0] < 0).any() and (r[1] >= hw[0]).any() for r in recs)
    _model_rate(recs, hw, mode)
    f, models = _filter(S, hw, mode)
    for parts in _consecutive(recs, sizes):
        _call(f, models, parts, 5000)
    assert f.errors()[0] > 0


@gpu
@pytest.mark.parametrize("mode", M.MODES)
def test_input_dtypes_and_signed_polarities(mode):
    hw = (12, 16)
    rec = M.recording(5, 1500, *hw, signed_p=True)
    assert set(rec[2].tolist()) == {-1, 1}
    want, _m = _model_rate([rec], hw, mode)
    for dxy, dt in ((torch.int16, torch.int64), (torch.int32, torch.int64), (torch.int64, torch.int64)):
        f, models = _filter(1, hw, mode)
        got = _call(f, models, [rec], 1500 + 13, dxy=dxy, dt=dt)
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
    small = M.recording(6, 1500, *hw, t_start=1000)               # int32 times cannot start above 2^33
    _model_rate([small], hw, mode)
    f, models = _filter(1, hw, mode)
    _call(f, models, [small], 1500, dxy=torch.int16, dt=torch.int32)


@gpu
@pytest.mark.parametrize("radius", [2, 3])
def test_activity_radius(radius):
    hw = (12, 16)
    recs = [M.recording(20 + s, n, *hw) for s, n in enumerate((2000, 300))]
    thr = M.thresholds(*hw)["activity"] // radius ** 2            # more pixels count: the threshold goes down to stay inside the band
    r1, _m = M.run(recs, *hw, mode="activity", threshold_us=thr, radius=1)
    rr, _m = _model_rate(recs, hw, "activity", threshold_us=thr, radius=radius)
    assert len(rr[0][0]) > len(r1[0][0])                            # the radius matters on this recording
    f, models = _filter(2, hw, "activity", threshold_us=thr, radius=radius)
    _call(f, models, recs, 2000)


@gpu
@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("hw", [(5, 7), (48, 64)], ids=["5x7", "48x64"])
def test_chunk_rule_cut_anywhere_equals_one_call(hw, mode):
    S, N, TIE = 3, 5000, 2000
    recs = [M.recording(30 + s, N, *hw) for s in range(S)]
    for s, r in enumerate(recs):                                    # events TIE and TIE + 1: one pixel, one microsecond, polarities differ
        r[0][TIE:TIE + 2], r[1][TIE:TIE + 2], r[2][TIE:TIE + 2] = 2 + s, 3, (1, 0)
        r[3][TIE:TIE + 2] = r[3][:TIE + 2].max()
    whole, ref = _model_rate(recs, hw, mode)
    f, models = _filter(S, hw, mode)
    _call(f, models, recs, N)
    one = [v.clone() for v in (f.surface, f.t_last, f.seen, f.kept, f.err)]
    # chunks of 0, 1 and 64 events, a cut between the two tied events, an empty chunk in the middle, a last chunk of one event
    for cuts in ([0, 1, 65, TIE + 1, 3000, 3000, N - 1], [64, 128, 129, TIE + 1, TIE + 2, 4097]):
        edges = [0] + cuts + [N]
        g, gm = _filter(S, hw, mode)
        parts_out = []
        for a, b in zip(edges[:-1], edges[1:]):
            parts_out.append(_call(g, gm, [tuple(c[a:b] for c in r) for r in recs], max(np.diff(edges)) + 3))
        for s in range(S):
            for k in range(4):
                assert np.array_equal(np.concatenate([po[s][k] for po in parts_out]), whole[s][k]), (s, k)
        for a, b in zip(one, (g.surface, g.t_last, g.seen, g.kept, g.err)):
            assert torch.equal(a, b)
        _state_equals(g, ref)


@gpu
@pytest.mark.parametrize("how", ["tensor", "host"])
def test_reset_of_one_row_in_mid_recording(how):
    hw, mode, S = (12, 16), "contrast", 3
    recs = [M.recording(40 + s, 1200, *hw) for s in range(S)]
    second = M.recording(49, 600, *hw, t_start=5000)                # row 1's new recording: a clock far below the first one's
    f, models = _filter(S, hw, mode)
    first = _call(f, models, [tuple(c[:600] for c in r) for r in recs], 600)
    parts = [tuple(c[600:] for c in recs[0]), second, tuple(c[600:] for c in recs[2])]
    if how == "tensor":
        nxt = _call(f, models, parts, 600, reset=[0, 1, 0])
    else:
        f.reset(streams=[1])
        models[1].reset()
        _state_equals(f, models)
        nxt = _call(f, models, parts, 600)
    assert int(nxt[1][3].min()) < 10 ** 6 and f.seen.cpu().tolist() == [1200, 600, 1200]
    fresh = M.FilterModel(*hw, mode, M.thresholds(*hw)[mode])
    assert all(np.array_equal(a, b) for a, b in zip(fresh.push(*second)[:4], nxt[1]))
    _in_band(sum(len(o[s][0]) for o in (first, nxt) for s in range(S)), 3600)
    (w0, w2), _m = M.run([recs[0], recs[2]], *hw, mode=mode, threshold_us=M.thresholds(*hw)[mode])      # the other rows: undisturbed
    for s, w in ((0, w0), (2, w2)):
        assert all(np.array_equal(np.concatenate([first[s][k], nxt[s][k]]), w[k]) for k in range(4))
    f.reset()
    assert (f.surface == -1).all() and f.errors() == (0,) and not f.t_last.any() and not f.seen.any() and not f.kept.any()


def _dat_rows(hw):
    """row 0: the fixture's records (clock around 2^31, events off the sensor, backwards times); row 1: a recording packed by the model"""
    F = np.load(os.path.join(GOLDEN, "dat_events.npz"))
    x, y, p, t = M.recording(50, 4000, *hw, t_start=300)
    x, y = np.maximum(x, 0), np.maximum(y, 0)                       # a record has no sign
    rec1 = QM.encode_dat(x, y, p, t, high_bits=np.arange(4000) % 8)
    return [F["records"], rec1], [tuple(F[k].astype(np.int64) for k in "xypt"), (x, y, p, t)]


@gpu
@pytest.mark.parametrize("mode,thr", [("activity", 300), ("contrast", 4000)])
def test_packed_records_equal_the_columns_path(mode, thr):
    hw = (48, 80)
    recs, rows = _dat_rows(hw)
    want, _m = _model_rate(rows, hw, mode, threshold_us=thr)
    buf = np.tile(np.asarray([[123, 1 | 1 << 14 | 1 << 28]], np.int32), (2, 4000 + 5, 1))
    for s, r in enumerate(recs):
        buf[s, :len(r)] = r
    counts = _i64([len(r) for r in recs])
    fd, md = _filter(2, hw, mode, threshold_us=thr)
    out = [v.clone() for v in fd.filter_dat(torch.from_numpy(buf).cuda(), counts)]
    _out_equals(out, want)
    fc, mc = _filter(2, hw, mode, threshold_us=thr)
    _call(fc, mc, rows, 4000 + 5)
    _state_equals(fd, mc)
    assert fd.errors()[0] > 0 and int(out[3][0, 0]) >= 2 ** 31 - 10 ** 4


# ------------------------------------------------------------------------------------------------------------------ the queue

_QKW = dict(bins=4, count_cutoff=10, duration_us=400)


def _queue_rows(hw, S=2, n=1500):
    """recordings inside the sensor (an encoder would clamp the others), clocks from 1000 (a fresh decoder's wrap base is then 0)"""
    rows = []
    for s in range(S):
        x, y, p, t = M.recording(60 + s, n - 200 * s, *hw, t_start=1000)
        rows.append((np.clip(x, 0, hw[1] - 1), np.clip(y, 0, hw[0] - 1), p, np.maximum.accumulate(t)))
    return rows


def _ends(rows, T=3):
    return _i64([[int(r[3][-1]) - 150 * (T - 1 - k) for r in rows] for k in range(T)])


@gpu
@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("mode", M.MODES)
def test_filtered_queue_gives_the_frames_of_the_models_kept_events(mode, ds):
    from sast_amd import _lib
    from sast_amd.events import EventQueue, Evt2Encoder, Evt3Encoder
    hw, S = (12, 16), 2
    rows = _queue_rows(hw)
    kept, _m = _model_rate(rows, hw, mode)
    kw = dict(_QKW, height=hw[0], width=hw[1], downsample_by_2=ds)
    ends = _ends(rows)
    plain = EventQueue(S, 4000, **kw)
    assert plain.filter is None
    kcols, kcounts = _chunk(kept, 1500)
    plain.push(*kcols, kcounts)
    want = plain.frames(ends, check=True)
    cols, counts = _chunk(rows, 1500)
    unfiltered = EventQueue(S, 4000, filter=None, **kw)
    unfiltered.push(*cols, counts)
    today = unfiltered.frames(ends, check=True)
    assert int(want.count_nonzero()) > 0 and not torch.equal(want, today)
    recs = torch.from_numpy(np.stack([np.concatenate([QM.encode_dat(*r), np.zeros((1500 - len(r[0]), 2), np.int32)]) for r in rows])).cuda()
    w3, n3 = (v.clone() for v in Evt3Encoder(S)(*cols, counts))
    w20, n20 = (v.clone() for v in Evt2Encoder(S, version="2.0")(*cols, counts))
    w21, n21 = (v.clone() for v in Evt2Encoder(S, version="2.1")(*cols, counts))
    pushes = {"push": lambda q: q.push(*cols, counts), "push_dat": lambda q: q.push_dat(recs, counts),
              "push_evt3": lambda q: q.push_evt3(w3, n3), "push_evt2": lambda q: q.push_evt2(w20, n20),
              "push_evt2 2.1": lambda q: q.push_evt2(w21, n21, version="2.1")}
    lib = _lib.lib()
    for name, push in pushes.items():
        f, _models = _filter(S, hw, mode)
        q = EventQueue(S, 4000, filter=f, **kw)
        before = lib.sast_launch_count()
        push(q)
        decode = 0 if name in ("push", "push_dat") else 2
        assert lib.sast_launch_count() - before == decode + f.FILTER_LAUNCHES + EventQueue.PUSH_LAUNCHES, name
        assert torch.equal(q.frames(ends, check=True), want), name
        assert f.kept.cpu().tolist() == [len(k[0]) for k in kept] and f.seen.cpu().tolist() == [len(r[0]) for r in rows], name
        q.reset(streams=[0])                                        # reaches the filter
        assert int(f.seen[0]) == 0 and int(f.seen[1]) > 0 and (f.surface[0] == -1).all() and (f.surface[1] >= 0).any(), name
    before = lib.sast_launch_count()
    unfiltered.push(*cols, counts)
    assert lib.sast_launch_count() - before == EventQueue.PUSH_LAUNCHES


@gpu
def test_filter_push_and_frames_in_one_graph():
    """captured once after a warm-up, replayed on new chunks, counts, ends and a reset flag written into the same tensors == eager"""
    from sast_amd.events import EventQueue
    hw, S, cap, mode = (12, 16), 2, 500, "activity"
    rows = _queue_rows(hw, n=1200)
    other = M.recording(77, 400, *hw, t_start=200)
    _model_rate(rows + [other], hw, mode)
    steps = [((rows[0], 0, 500), (rows[1], 0, 300), (0, 0)), ((rows[0], 500, 1000), (rows[1], 300, 600), (0, 0)),
             ((other, 0, 400), (rows[1], 600, 900), (1, 0))]      # at the third step row 0 starts a new recording
    bufs = [torch.zeros(S, cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    counts, ends, rst = _i64([0] * S), torch.zeros(2, S, dtype=torch.int64, device="cuda"), _u8([0] * S)

    def load(step):
        e = []
        for s, (rec, lo, hi) in enumerate(step[:2]):
            for buf, a, g in zip(bufs, rec, _GARBAGE):
                buf[s].fill_(g)
                buf[s, :hi - lo].copy_(torch.from_numpy(a[lo:hi]))
            top = int(np.maximum.accumulate(rec[3])[hi - 1]) - 1
            e.append((top - 200, top))
        counts.copy_(_i64([hi - lo for _r, lo, hi in step[:2]]))
        ends.copy_(torch.tensor(e, dtype=torch.int64).t())
        rst.copy_(_u8(step[2]))

    def make():
        f, models = _filter(S, hw, mode)
        return EventQueue(S, 1400, filter=f, height=hw[0], width=hw[1], **_QKW), f, models

    def call(q):
        q.push(*bufs, counts, reset=rst)
        return q.frames(ends)

    qe, fe, models = make()
    eager = []
    for st in steps:
        load(st)
        fr = call(qe)
        for s, (m, (rec, lo, hi)) in enumerate(zip(models, st[:2])):
            m.push(*(c[lo:hi] for c in rec), reset=bool(st[2][s]))
        _state_equals(fe, models)
        eager.append((fr.clone(), [v.clone() for v in (fe.surface, fe.t_last, fe.seen, fe.kept, fe.counts, qe.count, qe.t_last)]))
    assert int(eager[2][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    q, f, _models = make()
    load(steps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(q)                                                     # the warm-up allocates; a capture without it raises (F.not_capturing)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(q)
    q.reset()                                                       # the warm-up's step is undone: queue and filter start over
    for st, (fr, state) in zip(steps, eager):
        load(st)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, fr)
        for u, v in zip(state, (f.surface, f.t_last, f.seen, f.kept, f.counts, q.count, q.t_last)):
            assert torch.equal(u, v)
    assert f.errors() == fe.errors() and q.errors() == qe.errors()


@gpu
def test_online_detector_on_a_filtered_queue_eager_and_replayed(detector):  # noqa: F811
    from sast_amd.events import EventFilter
    from sast_amd.online import OnlineDetector
    rounds, _recs, _e = TO._session(2, seed=41, reset_round=2, max_rounds=4)

    def online():
        f = EventFilter(TO.S, mode="activity", threshold_us=4000, radius=3, **TO.GEO)
        return OnlineDetector(detector, TO._queue(filter=f), windows_per_step=2, max_det=TO.MAX_DET, conf_thre=TO.CONF, nms_thre=TO.NMS), f

    eager, fe = online()
    want = []
    for parts, reset, final, *_m in rounds:
        TO._push(eager, parts, reset, final)
        want.append(eager.drain())
    models = [M.FilterModel(mode="activity", threshold_us=4000, radius=3, **TO.GEO) for _ in range(TO.S)]
    for parts, reset, *_m in rounds:
        for m, part, r in zip(models, parts, reset):
            m.push(*part, reset=bool(r))
    _in_band(sum(m.kept for m in models), sum(m.seen for m in models))
    assert fe.kept.cpu().tolist() == [m.kept for m in models]
    od, f = online()
    cols, counts = TO._chunk(rounds[0][0])
    reset, final = TO._u8(rounds[0][1]), TO._u8(rounds[0][2])
    od.push(*cols, counts, reset, final)
    TO._same(od.drain(), want[0])
    od.capture()
    for (parts, rst, fin, *_m), expect in zip(rounds[1:], want[1:]):
        new_cols, new_counts = TO._chunk(parts)
        for dst, src in zip(cols + [counts, reset, final], new_cols + [new_counts, TO._u8(rst), TO._u8(fin)]):
            dst.copy_(src)
        od.replay()
        TO._same(od.drain(), expect)
    assert sum(len(a) for step in want for _s, a in step) > 0 and any(r[1].any() for r in rounds[1:])
    assert torch.equal(f.surface, fe.surface) and torch.equal(f.kept, fe.kept) and od.errors() == eager.errors()
