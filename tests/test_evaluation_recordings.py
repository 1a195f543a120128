"""`PropheseeEvaluator.add_recordings` and `online.DetectionLog` (sast_amd/evaluation.py, sast_amd/online.py, csrc/k_eval.hip).

Yardsticks: tests/recording_model.py (numpy; pinned to the reference's filter_boxes + _match_times by tests/test_recording_model.py on
tests/golden/eval_recordings.npz) for the tables, tests/coco_reference.py for the precision table and the six numbers.
Bounds: tables, records and the precision table are exact; the six summaries are means of at most 3030 values in [0, 1], so any
summation order stays within 3030 * 2^-53 ~ 3.4e-13 < SUMMARY_TOL = 1e-12 (the bar of tests/test_evaluation.py).
Inputs on the device carry NaN / huge words behind every count."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import make_golden_eval as GE  # noqa: E402
import make_golden_eval_recordings as G  # noqa: E402
import recording_model as RM  # noqa: E402
import test_online_detector as TOD  # noqa: E402
from test_recording_model import fixture_rows  # noqa: E402
from sast_amd import evaluation as E  # noqa: E402

gpu = pytest.mark.gpu
detector = TOD.detector
SUMMARY_TOL = 1e-12
NAN_BITS, HUGE_BITS = 0x7fc00000, 0x7f7fffff
TABLE_KEYS = ("image_t", "gt_image_id", "gt_category_id", "gt_bbox", "gt_area", "dt_image_id", "dt_category_id", "dt_score", "dt_bbox",
              "dt_area")


def _pack(recs, extra=3, cuda=True):
    """a list of record arrays -> (int32 [S, cap, 10] with garbage behind each row's records, int64 [S])"""
    cap = max(len(r) for r in recs) + extra
    w = np.empty((len(recs), cap, 10), np.int32)
    w[..., 0::2], w[..., 1::2] = NAN_BITS, HUGE_BITS
    for s, r in enumerate(recs):
        w[s, :len(r)] = RM.words(r)
    t, n = torch.from_numpy(w), torch.tensor([len(r) for r in recs], dtype=torch.int64)
    return (t.cuda(), n.cuda()) if cuda else (t, n)


def _feed(ev, rows, **kw):
    gt, n_gt = _pack([g for g, _d in rows])
    dt, n_dt = _pack([d for _g, d in rows])
    ev.add_recordings(gt, n_gt, dt, n_dt, **kw)


def _evaluator(**caps):
    kw = dict(max_images=64, max_detections=4096, max_labels_per_frame=12)
    kw.update(caps)
    return E.PropheseeEvaluator("gen1", False, **kw)


def _model(**caps):
    return RM.Model(G.DIAG, G.SIDE, **caps)


def _same_tables(got, want):
    for k in TABLE_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _snapshot(ev):
    """everything the buffer holds: the state words, the tables and the per-detection records"""
    blob = ev.export_buffer()
    return {k: v.cpu().numpy() for k, v in blob.items() if isinstance(v, torch.Tensor)}


def _same_buffers(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _records(rows):
    r = RM.records(len(rows))
    for i, row in enumerate(rows):
        r[i] = row
    return r


def _small_rows(n_crowd=40):
    """one recording, three label timestamps; the middle window holds n_crowd detection records"""
    rs = np.random.RandomState(9)
    gt = _records([(t, 20 + 10 * i, 30, 40 + i, 50, i % 2, 0, 1.0) for t in (600000, 800000, 1000000) for i in range(2)])
    dets = [(600000, 22, 31, 40, 48, 0, 0, 0.5)] * 3
    dets += [(760000 + 2000 * i, 20 + rs.randint(20), 30, 30 + rs.randint(20), 50, i % 2, 0, rs.randint(1, 9) / 8.0) for i in range(n_crowd)]
    dets += [(1000000, 31, 30, 41, 50, 1, 0, 0.25)] * 2
    return [(gt, _records(dets))]


# ------------------------------------------------------------------------------------------------------------------- without a GPU
def test_add_recordings_refuses_bad_arguments_before_any_device_work():
    ev = _evaluator()
    rows = fixture_rows()
    gt, n_gt = _pack([g for g, _d in rows], cuda=False)
    dt, n_dt = _pack([d for _g, d in rows], cuda=False)
    with pytest.raises(TypeError, match="gt must be a contiguous int32 tensor of shape \\[S, Gcap, 10\\]"):
        ev.add_recordings(gt.float(), n_gt, dt, n_dt)
    with pytest.raises(ValueError, match="gt must be"):
        ev.add_recordings(gt[..., :9], n_gt, dt, n_dt)
    with pytest.raises(TypeError, match="n_gt must be a contiguous int64 tensor of shape \\[3\\]"):
        ev.add_recordings(gt, n_gt.int(), dt, n_dt)
    with pytest.raises(ValueError, match="n_gt must be"):
        ev.add_recordings(gt, n_gt[:2], dt, n_dt)
    with pytest.raises(ValueError, match="dt must be .*\\[S=3, Dcap, 10\\]"):
        ev.add_recordings(gt, n_gt, dt[:2], n_dt)
    with pytest.raises(ValueError, match="dt must be"):
        ev.add_recordings(gt, n_gt, dt.transpose(0, 1), n_dt)
    with pytest.raises(TypeError, match="n_dt must be"):
        ev.add_recordings(gt, n_gt, dt, n_dt.double())
    with pytest.raises(ValueError, match="time_tol_us must be >= 0"):
        ev.add_recordings(gt, n_gt, dt, n_dt, time_tol_us=-1)
    for bad in (0, 8193):
        with pytest.raises(ValueError, match="max_window_detections must be in 1 .. 8192"):
            ev.add_recordings(gt, n_gt, dt, n_dt, max_window_detections=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.add_recordings(gt, n_gt, dt, n_dt)
    assert not ev.has_data()


def test_detection_log_refuses_bad_arguments():
    from sast_amd.online import DetectionLog, OnlineDetector
    with pytest.raises(ValueError):
        DetectionLog(0, 8)
    with pytest.raises(ValueError):
        DetectionLog(3, 0)
    log = DetectionLog(3, 8)
    rec, cnt = torch.zeros(3, 5, 40, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="records must be"):
        log.append(rec[:2], cnt)
    with pytest.raises(ValueError, match="counts must be"):
        log.append(rec, cnt.long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        log.append(rec, cnt)
    log.clear()                                                    # nothing allocated: nothing to do
    assert log.records is None

    class _Det:
        training = False

        class yolox_head:
            num_classes = 2

    with pytest.raises(ValueError, match="log must be a DetectionLog"):
        OnlineDetector(_Det(), TOD._queue(), windows_per_step=2, log=DetectionLog(2, 8))
    assert OnlineDetector(_Det(), TOD._queue(), windows_per_step=2).log is None


def test_recording_entry_points_declared_bound_and_exported():
    import ctypes as C
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evrec_") or n.startswith("sast_detlog_")]
    assert sorted(names) == ["sast_detlog_append", "sast_evrec_add", "sast_evrec_ws_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    a, r, d = _lib.SastEvalArgs(), _lib.SastEvRecArgs(), _lib.SastDetLogArgs()
    assert lib.sast_evrec_add(C.byref(a), C.byref(r), None) == -22 and lib.sast_evrec_add(None, None, None) == -22
    assert lib.sast_detlog_append(C.byref(d), None) == -22 and lib.sast_detlog_append(None, None) == -22
    assert lib.sast_evrec_ws_bytes(0, 8) == 0 and lib.sast_evrec_ws_bytes(1, 0) == 0 and lib.sast_evrec_ws_bytes(65535, 1 << 20) == 0
    assert lib.sast_evrec_ws_bytes(3, 16) == 4 * (3 * 16 * 17 + 2 * 3)
    assert _lib.EVAL_STATE_WORDS == 32 and _lib.EVAL_MAX_CLASSES * _lib.EVAL_AREAS + 12 == 28     # words 28.. are behind [K][4]


# ------------------------------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("tol", G.TOLS)
def test_tables_precision_and_summaries_equal_the_model(tol):
    from conftest import record_error
    rows = fixture_rows()
    ev = _evaluator()
    _feed(ev, rows, time_tol_us=tol)
    m = _model()
    m.add_recordings(rows, tol=tol)
    want = m.tables()
    _same_tables(ev.tables(), want)
    got = ev.evaluate_buffer(240, 304)
    stats, prec = CR.evaluate(*RM.coco_inputs(want), G.K)
    p = ev.precision().cpu().numpy()
    diff = p != prec
    print("tol", tol, "precision entries that differ:", int(diff.sum()), "of", p.size)
    assert p.shape == prec.shape == (10, 101, G.K, 4) and not diff.any(), np.argwhere(diff)[:8]
    for k in CR.OUT_KEYS:
        err = abs(got[k] - stats[k])
        print("tol", tol, k, got[k], stats[k], err)
        record_error("test_tables_precision_and_summaries_equal_the_model", f"tol {tol} {k}", err, 1.0, SUMMARY_TOL)
        assert err <= SUMMARY_TOL, (k, got[k], stats[k])
    assert not any(int(v) for v in ev._state[8:11]) and ev._state[28] == 0 and ev._state[29] == 0 and ev._state[11] == 1


def _frames_as_recording():
    """gen1 frames of tests/golden/make_golden_eval.py with distinct fp32-exact timestamps below 2^24 us"""
    labels, counts, det, n_det = (a.copy() for a in GE.case_inputs("gen1"))
    N = labels.shape[0]
    t = np.array([400000, 500000] + [600000 + 50000 * n for n in range(2, N)], np.int64)
    assert len(set(t)) == N and t.max() < 2 ** 24
    for n in range(N):
        labels[n, :counts[n], 0] = t[n]
    return labels, counts, det, n_det, t


@gpu
def test_time_tol_zero_equals_the_frame_form_bit_for_bit():
    from sast_amd.online import export_detections
    labels, counts, det, n_det, t = _frames_as_recording()
    N, A = det.shape[0], det.shape[1]
    frames = _evaluator()
    frames.add(*(torch.from_numpy(a).cuda() for a in (labels, counts, det, n_det)))
    records = torch.zeros(N, A, 40, dtype=torch.uint8).cuda()
    n_rec, cut = torch.zeros(N, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    export_detections(torch.from_numpy(det).cuda(), torch.from_numpy(n_det).cuda(), torch.from_numpy(t).cuda(),
                      torch.ones(N, dtype=torch.uint8).cuda(), records, n_rec, cut)
    assert int(cut.item()) == 0 and n_rec.cpu().tolist() == n_det.tolist()
    raw = records.cpu().numpy()
    dt = np.concatenate([raw[n, :n_det[n]].reshape(-1).view(RM.BBOX_DTYPE) for n in range(N)])
    gt = _records([(int(t[n]),) + tuple(labels[n, i, 1:5]) + (int(labels[n, i, 5]), 0, labels[n, i, 6]) for n in range(N) for i in range(counts[n])])
    rec = _evaluator()
    _feed(rec, [(gt, dt)], time_tol_us=0, max_window_detections=A)
    a, b = _snapshot(frames), _snapshot(rec)
    assert a["state"][0] > 10 and a["state"][3] > 100
    _same_buffers(a, b)
    assert frames.evaluate_buffer(240, 304) == rec.evaluate_buffer(240, 304)
    assert np.array_equal(frames.precision().cpu().numpy().view(np.int64), rec.precision().cpu().numpy().view(np.int64))


@gpu
def test_a_window_over_max_window_detections_is_refused_alone():
    rows = _small_rows(40)
    m, free = _model(), _model()
    m.add_recordings(rows, max_window=32)
    free.add_recordings(rows)
    assert m.refused["max_window_detections"] == 1 and sum(m.refused.values()) == 1 and len(m.image_t) == 2 and len(free.image_t) == 3
    assert max(n for *_x, n in RM.windows(*rows[0], 50000, G.DIAG, G.SIDE)) == 40
    ev = _evaluator()
    _feed(ev, rows, max_window_detections=32)
    _same_tables(ev.tables(), m.tables())
    with pytest.raises(OverflowError, match="max_window_detections=32"):
        ev.evaluate_buffer(240, 304)
    assert ev._state[28] == 1 and ev._state[29] == 0 and not ev._state[8:11].any()
    ev = _evaluator()                                              # the limit itself fits
    _feed(ev, rows, max_window_detections=40)
    _same_tables(ev.tables(), free.tables())
    assert ev.evaluate_buffer(240, 304) is not None and ev._state[28] == 0


@gpu
@pytest.mark.parametrize("side", ["labels", "detections"])
def test_an_unsorted_row_adds_nothing_and_raises(side):
    rows = fixture_rows()
    g, d = rows[0][0].copy(), rows[0][1].copy()
    if side == "labels":
        g["t"][len(g) - 1] = g["t"][len(g) - 2] - 1
    else:
        d["t"][7] = d["t"][6] - 1
    bad = [(g, d), rows[2], _small_rows(5)[0]]
    m = _model()
    m.add_recordings(bad)
    assert m.refused["unsorted"] == 1 and sum(m.refused.values()) == 1 and len(m.image_t) > 3
    ev = _evaluator()
    _feed(ev, bad)
    _same_tables(ev.tables(), m.tables())
    with pytest.raises(ValueError, match="not sorted by t"):
        ev.evaluate_buffer(240, 304)
    assert ev._state[29] == 1 and ev._state[28] == 0 and not ev._state[8:11].any()
    with pytest.raises(RuntimeError):
        ev.precision()


@gpu
def test_capacity_refusals_behave_as_for_add():
    rows = fixture_rows()
    free = _model()
    free.add_recordings(rows)
    n_img, n_dt = len(free.image_t), len(free.dt)
    for caps, mcaps, key, word in ((dict(max_images=n_img - 2), dict(max_images=n_img - 2), "max_images", 8),
                                   (dict(max_detections=n_dt - 1), dict(max_detections=n_dt - 1), "max_detections", 9),
                                   (dict(max_labels_per_frame=3), dict(max_labels=3), "max_labels_per_frame", 10)):
        m = _model(**mcaps)
        m.add_recordings(rows)
        assert m.refused[key] >= 1 and sum(m.refused.values()) == m.refused[key]        # the model stays inside every other cap
        ev = _evaluator(**caps)
        _feed(ev, rows)
        _same_tables(ev.tables(), m.tables())
        with pytest.raises(OverflowError, match=f"{key}={caps[key]}"):
            ev.evaluate_buffer(240, 304)
        assert ev._state[word] == m.refused[key] and sum(int(ev._state[w]) for w in (8, 9, 10, 28, 29)) == m.refused[key]
    ev = _evaluator(max_images=n_img, max_detections=n_dt, max_labels_per_frame=max(len(g) for _t, g, _d, _n in
                                                                                   RM.windows(*rows[0], 50000, G.DIAG, G.SIDE)))
    _feed(ev, rows)                                                # an exact fit
    _same_tables(ev.tables(), free.tables())
    assert ev.evaluate_buffer(240, 304) is not None


@gpu
def test_rows_split_over_calls_give_the_same_buffer():
    rows = fixture_rows() + _small_rows(12)
    whole = _evaluator()
    _feed(whole, rows)
    want = _snapshot(whole)
    for cuts in ([1], [2, 3], [1, 2, 3]):
        ev = _evaluator()
        for lo, hi in zip([0] + cuts, cuts + [len(rows)]):
            _feed(ev, rows[lo:hi])
        got = _snapshot(ev)
        assert got["state"][11] == len(cuts) + 1
        got["state"][11] = want["state"][11]                       # the add counter is the one word that counts calls
        _same_buffers(got, want)
    # slices of one packed tensor: rows that do not start at the allocation
    gt, n_gt = _pack([g for g, _d in rows])
    dt, n_dt = _pack([d for _g, d in rows])
    ev = _evaluator()
    ev.add_recordings(gt[:2], n_gt[:2], dt[:2], n_dt[:2])
    ev.add_recordings(gt[2:], n_gt[2:], dt[2:], n_dt[2:])
    got = _snapshot(ev)
    got["state"][11] = want["state"][11]
    _same_buffers(got, want)


@gpu
def test_add_then_add_recordings_then_merge_carries_everything():
    rows = fixture_rows()
    d = rows[0][1].copy()
    d["t"][3] = d["t"][2] - 1
    rows = rows + [(rows[0][0], d)]                                # a fourth, unsorted row: word 29
    frames = [torch.from_numpy(a).cuda() for a in GE.case_inputs("gen1")]
    one = _evaluator()
    one.add(*frames)
    _feed(one, rows, max_window_detections=100)                    # the crowded window is refused: word 28
    one.add(*frames)
    first, second, third = _evaluator(), _evaluator(), _evaluator()
    first.add(*frames)
    _feed(second, rows, max_window_detections=100)
    third.add(*frames)
    first.merge(second)
    first.merge(third)
    a, b = _snapshot(one), _snapshot(first)
    assert a["state"][28] == 1 and a["state"][29] == 1 and a["state"][11] == 3
    _same_buffers(a, b)
    for ev in (one, first):
        with pytest.raises(ValueError, match="not sorted by t"):
            ev.evaluate_buffer(240, 304)
    # without the unsorted row both evaluate, to the same bits; images of the two forms are numbered in call order
    one, first, second = _evaluator(), _evaluator(), _evaluator()
    one.add(*frames)
    _feed(one, rows[:3])
    first.add(*frames)
    _feed(second, rows[:3])
    first.merge(second)
    _same_buffers(_snapshot(one), _snapshot(first))
    assert one.evaluate_buffer(240, 304) == first.evaluate_buffer(240, 304)
    assert np.array_equal(one.precision().cpu().numpy().view(np.int64), first.precision().cpu().numpy().view(np.int64))
    tab = one.tables()
    m = _model()
    m.add_recordings(rows[:3])
    n_frames_images = len(tab["image_t"]) - len(m.image_t)
    assert n_frames_images > 0 and np.array_equal(tab["image_t"][n_frames_images:], m.tables()["image_t"])


@gpu
def test_captured_add_recordings_replays_on_new_records_and_counts():
    rows_a = fixture_rows()
    rows_b = [rows_a[2], _small_rows(20)[0], rows_a[0]]
    cap_g, cap_d = max(len(g) for g, _d in rows_a) + 3, max(len(d) for _g, d in rows_a) + 3

    def packed(rows):
        gt, n_gt = _pack([g for g, _d in rows], extra=cap_g - max(len(g) for g, _d in rows))
        dt, n_dt = _pack([d for _g, d in rows], extra=cap_d - max(len(d) for _g, d in rows))
        return gt, n_gt, dt, n_dt

    want = {}
    for name, rows in (("a", rows_a), ("b", rows_b)):
        ev = _evaluator()
        ev.add_recordings(*packed(rows))
        want[name] = (_snapshot(ev), ev.evaluate_buffer(240, 304), ev.precision().cpu().numpy())
    assert not np.array_equal(want["a"][0]["img_t"], want["b"][0]["img_t"])
    ev = _evaluator()
    static = packed(rows_a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.add_recordings(*static)                                 # the eager call: buffers, LDS attribute
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.add_recordings(*static)
    for name, rows in (("b", rows_b), ("a", rows_a), ("b", rows_b)):
        for dst, src in zip(static, packed(rows)):
            dst.copy_(src)
        ev.reset_buffer()
        g.replay()
        _same_buffers(_snapshot(ev), want[name][0])
        assert ev.evaluate_buffer(240, 304) == want[name][1]
        assert np.array_equal(ev.precision().cpu().numpy().view(np.int64), want[name][2].view(np.int64))


# ------------------------------------------------------------------------------------------------------------------ DetectionLog
def _per_stream(steps, S):
    out = [[] for _ in range(S)]
    for s, a in steps:
        out[s].append(a)
    return [np.concatenate(v) if v else RM.records(0) for v in out]


def _log_rows(log):
    rec, n = log.records.cpu().numpy(), log.counts.cpu().tolist()
    return [RM.from_words(rec[s, :n[s]]) for s in range(log.num_streams)]


def _logged_session(detector, captured, capacity=4096, reset_round=2):
    from sast_amd.online import DetectionLog
    rounds, _recs, _e = TOD._session(2, seed=41, reset_round=reset_round, max_rounds=4)
    rounds[3][2][2] = 1                                            # row 2 finishes early: its last windows are given
    log = DetectionLog(TOD.S, capacity)
    od = TOD._online(detector, log=log)
    steps = []
    cols, counts = TOD._chunk(rounds[0][0])
    reset, final = TOD._u8(rounds[0][1]), TOD._u8(rounds[0][2])
    od.push(*cols, counts, reset, final)
    steps += od.drain()
    if captured:
        od.capture()
    for parts, rst, fin, *_m in rounds[1:]:
        if rst.any():                                              # a new recording in that row: its log starts over, and so does the model's
            log.clear(np.nonzero(rst)[0])
            steps = [(s, a) for s, a in steps if not rst[s]]
        if captured:
            new_cols, new_counts = TOD._chunk(parts)
            for dst, src in zip(cols + [counts, reset, final], new_cols + [new_counts, TOD._u8(rst), TOD._u8(fin)]):
                dst.copy_(src)
            od.replay()
        else:
            TOD._push(od, parts, rst, fin)
        steps += od.drain()
    return log, steps, rounds


@gpu
@pytest.mark.parametrize("captured", [False, True])
def test_detection_log_equals_the_concatenated_drain(detector, captured):
    log, steps, rounds = _logged_session(detector, captured)
    assert any(not r[4].all() for r in rounds) and any(r[1].any() for r in rounds[1:])          # rows not due; a reset
    want = _per_stream(steps, TOD.S)
    got = _log_rows(log)
    assert sum(len(w) for w in want) > 0 and int(log.dropped.item()) == 0
    for s in range(TOD.S):
        assert RM.same_records(got[s], want[s]), s
        assert RM.is_sorted(got[s])


@gpu
def test_a_log_too_small_drops_whole_steps_and_counts_them(detector):
    _big, steps, _rounds = _logged_session(detector, False, reset_round=99)
    sizes = [len(a) for _s, a in steps if len(a)]
    cap = max(sizes) + min(sizes)                                  # every step fits an empty log, not all of them fit one after another
    log, steps, _rounds = _logged_session(detector, False, capacity=cap, reset_round=99)
    want, dropped = [[] for _ in range(TOD.S)], 0
    for s, a in steps:
        if len(a) and sum(len(x) for x in want[s]) + len(a) > cap:
            dropped += 1
        elif len(a):
            want[s].append(a)
    assert dropped > 0 and int(log.dropped.item()) == dropped
    for s, got in enumerate(_log_rows(log)):
        assert RM.same_records(got, np.concatenate(want[s]) if want[s] else RM.records(0)), s
    log.clear()
    assert int(log.dropped.item()) == 0 and log.counts.cpu().tolist() == [0] * TOD.S


@gpu
def test_the_log_costs_one_launch_per_step_and_none_without_it(detector):
    from sast_amd import _lib
    from sast_amd.online import DetectionLog
    rounds, _recs, _e = TOD._session(2, seed=41, reset_round=2, max_rounds=2)
    counts = []
    for log in (None, DetectionLog(TOD.S, 4096), None):
        od = TOD._online(detector, log=log)
        TOD._push(od, *rounds[0][:3])                              # the first push allocates
        before = _lib.lib().sast_launch_count()
        TOD._push(od, *rounds[1][:3])
        counts.append(_lib.lib().sast_launch_count() - before)
        od.drain()
        assert (od._offsets[4], len(od._slots)) == (TOD.S * 2 * (8 + 40 * TOD.MAX_DET + 4 + 1), 2)
    assert counts[0] == counts[2] and counts[1] == counts[0] + 2   # W = 2 steps: one sast_detlog_append each


# ------------------------------------------------------------------------------------------------------------------ end to end
@gpu
def test_events_to_map_with_no_record_on_the_host(detector):
    """synthetic events of two cameras -> OnlineDetector(log=) -> add_recordings against synthetic labels -> evaluate_buffer, equal
    to the model fed what drain() brought to the host"""
    from conftest import record_error
    from sast_amd.events import EventQueue
    from sast_amd.online import DetectionLog, OnlineDetector
    S, W, T0, n_ev = 2, 2, 600000, 400
    recs = [[c[:n_ev].copy() for c in TOD._recording(r)] for r in (TOD.FAST, TOD.SLOW_A)]
    for r in recs:
        r[3] = r[3] + (T0 - TOD.D)                                 # the filter drops everything at or before 0.5 s
    log = DetectionLog(S, 8192)
    od = OnlineDetector(detector, EventQueue(S, TOD.CAP, duration_us=TOD.D, **TOD.GEO), windows_per_step=W, max_det=TOD.MAX_DET,
                        conf_thre=0.05, nms_thre=TOD.NMS, first_end_us=T0, log=log)
    empty = [tuple(c[:0] for c in r) for r in recs]
    steps = []
    for k in range(40):
        cols, counts = TOD._chunk([tuple(r) for r in recs] if k == 0 else empty, cap=n_ev)
        od.push(*cols, counts, None, TOD._u8([1, 1]))
        steps += od.drain()
        if k > 0 and od.errors()[5] == 0:
            break
    assert od.errors()[5] == 0                                     # every window was given
    dets = _per_stream(steps, S)
    assert sum(len(d) for d in dets) >= 1 and all(RM.same_records(a, b) for a, b in zip(_log_rows(log), dets))
    rs = np.random.RandomState(17)
    gts = []
    for d in dets:                                                 # labels at some detection times and between them; boxes near detections
        ts = np.unique(d["t"])
        rows = []
        for t in sorted(set(ts[::3].tolist() + (ts[1::4] + 250).tolist())):
            near = d[np.abs(d["t"] - t) <= 1000]
            for i in range(1 + rs.randint(3)):
                b = near[rs.randint(len(near))] if len(near) and rs.rand() < 0.7 else None
                x, y, w, h = (b["x"], b["y"], b["w"], b["h"]) if b is not None else (rs.randint(100), rs.randint(70), 12 + rs.randint(40), 12 + rs.randint(40))
                rows.append((int(t), x + rs.randint(-2, 3), y, max(w, 11.0), max(h, 11.0), rs.randint(2) if b is None else int(b["class_id"]), 0, 1.0))
        gts.append(_records(rows))
    rows = list(zip(gts, dets))
    m = _model()
    m.add_recordings(rows, tol=1000)
    want = m.tables()
    assert not any(m.refused.values()) and len(want["image_t"]) > 4 and len(want["dt_score"]) > 0
    ev = E.PropheseeEvaluator("gen1", False, max_images=512, max_detections=1 << 16, max_labels_per_frame=8)
    gt, n_gt = _pack(gts)
    ev.add_recordings(gt, n_gt, log.records, log.counts, time_tol_us=1000, max_window_detections=2048)
    _same_tables(ev.tables(), want)
    got = ev.evaluate_buffer(128, 160)
    stats, prec = CR.evaluate(*RM.coco_inputs(want), 2)
    assert np.array_equal(ev.precision().cpu().numpy(), prec)
    for k in CR.OUT_KEYS:
        err = abs(got[k] - stats[k])
        print(k, got[k], stats[k], err)
        record_error("test_events_to_map_with_no_record_on_the_host", k, err, 1.0, SUMMARY_TOL)
        assert err <= SUMMARY_TOL
