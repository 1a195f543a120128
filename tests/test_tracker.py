"""sast_amd.tracking on the MI355X: the records and every state tensor of `DetectionTracker` against the sequential model
(tests/tracker_model.py), as bytes and integers, at the sizes where the kernel can go wrong: tables of 1, 5, 64, 65 and 128 slots,
1, 8 and 100 records per row, steps of 0, 63, 64 and 65 detections, rows that are not due, a reset half-way.  Box coordinates are
multiples of 0.25 and every step's boxes are jittered copies of the step before inside a small field, so most pairs are candidates and
the matching needs several mutual-best rounds.  Then the recording driver against the stepped run, and `OnlineDetector(tracker=...)`
end to end, eager and captured, with a `DetectionLog` behind it."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracker_model as TM  # noqa: E402
from test_tracker_model import mutual_best_rounds  # noqa: E402

from sast_amd.labels import BBOX_DTYPE  # noqa: E402

gpu = pytest.mark.gpu
S, STEPS = 3, 24
TARGETS = [20, 63, 64, 65, 0, 100, 40, 65, 0, 64, 63, 90, 7, 1, 65, 64, 0, 63, 100, 33, 64, 65, 63, 12]     # detections per step, before max_det
STATE = ("ids", "box", "cls", "last_t", "hits", "next_id", "counters")


def _due(k, s):
    return (1, k % 2 == 0, k % 3 != 0)[s]


def sequence(max_det, seed, duplicates=False, resets=True):
    """[(records uint8 [S, max_det, 40], counts, ends, due, reset)] per step.  Records past counts[s] and the rows that are not due hold
    random bytes; one step gives a count above max_det (the clamp) and one a negative one."""
    rng = np.random.RandomState(seed)
    live = [[] for _ in range(S)]
    steps = []
    for k in range(STEPS):
        rec = rng.randint(0, 256, size=(S, max_det, 40)).astype(np.uint8)
        counts, ends, due, reset = np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        for s in range(S):
            due[s], ends[s] = _due(k, s), 1000 * (k + 1) + s
            if resets:
                reset[s] = (s == 1 and k == 12) or (s == 2 and k == 9)                  # row 2's reset falls on a step it is not due
            if not due[s]:
                counts[s] = rng.randint(0, max_det + 1)
                continue
            n = min(TARGETS[(k + 5 * s) % STEPS], max_det)
            objs = [(x + rng.randint(-6, 7) * 0.25, y + rng.randint(-6, 7) * 0.25, w, h, c) for x, y, w, h, c in live[s]]
            rng.shuffle(objs)
            objs = objs[:max(n - rng.randint(0, 4), 0)]                                 # deaths
            while len(objs) < n:                                                        # births
                if duplicates:
                    objs.append((rng.randint(0, 4) * 8.0, 4.0, 16.0, 12.0, 1))
                else:
                    objs.append((rng.randint(0, 120) * 0.25, rng.randint(0, 120) * 0.25, rng.randint(24, 96) * 0.25, rng.randint(24, 96) * 0.25,
                                 rng.randint(3)))
            if duplicates:                                                              # snapped to a grid of 4: a handful of distinct boxes
                objs = [(float(np.floor(x / 4 + 0.5)) * 4.0, float(np.floor(y / 4 + 0.5)) * 4.0, w, h, c) for x, y, w, h, c in objs]
            rng.shuffle(objs)
            live[s] = objs
            r = rec[s].reshape(-1).view(BBOX_DTYPE)
            for j, (x, y, w, h, c) in enumerate(objs):
                r[j] = (ends[s], x, y, w, h, c, rng.randint(0, 2 ** 31), 0.5 if duplicates else rng.randint(1, 65) / 64.0)
            counts[s] = n
            if k == 7 and s == 0 and n == max_det:
                counts[s] = max_det + 5                                                 # clamped, nothing past the row is read
            if k == 5 and s == 0 and n >= 2:
                r[1]["x"] = np.nan                                                      # a NaN box: never a candidate, born as it is
        if k == 13:
            counts[0], due[0] = -2, 1
        steps.append((rec, counts, ends, due, reset))
    return steps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def assert_state(tr, model, where):
    want = model.state()
    for name in STATE:
        got = getattr(tr, name).cpu().numpy()
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (name, where)
        assert np.array_equal(_bits(got), _bits(want[name])), (name, where)


def run_both(steps, max_det, **kw):
    """the steps through `DetectionTracker.step` and through the model, compared after every step -> (tracker, model, the records after)"""
    from sast_amd.tracking import DetectionTracker
    tr, model = DetectionTracker(S, max_det, **kw), TM.TrackerModel(S, max_det, **kw)
    out, touched = [], 0
    for k, (rec, counts, ends, due, reset) in enumerate(steps):
        d_rec = _dev(rec)
        tr.step(d_rec, _dev(counts), _dev(ends), _dev(due), _dev(reset) if reset.any() or k % 2 else None)
        want = rec.copy()
        model.step([want[s].reshape(-1).view(BBOX_DTYPE) for s in range(S)], counts, ends, due, reset)
        got = d_rec.cpu().numpy()
        assert np.array_equal(got, want), k
        # the canaries, against the input itself: only bytes 28 .. 31 of the first m records of a due row may differ
        changed = got != rec
        for s in range(S):
            m = min(max(int(counts[s]), 0), max_det) if due[s] else 0
            assert not changed[s, m:].any() and not changed[s, :, :28].any() and not changed[s, :, 32:].any(), (k, s)
            touched += int(changed[s, :m].any(axis=1).sum())
        assert_state(tr, model, k)
        out.append(got)
    assert touched > 0
    return tr, model, out


# ------------------------------------------------------------------------------------------------------------------ the step driver

@gpu
@pytest.mark.parametrize("max_det", [1, 8, 100])
@pytest.mark.parametrize("max_tracks", [1, 5, 64, 65, 128])
def test_step_equals_the_model_in_records_and_state(max_tracks, max_det):
    agnostic = max_tracks in (5, 65)
    steps = sequence(max_det, seed=1000 * max_tracks + max_det)
    if max_det == 100:
        ms = {int(c) for _r, cnt, _e, due, _x in steps for c, d in zip(cnt, due) if d}
        assert {0, 63, 64, 65, 100} <= ms
    tr, model, _out = run_both(steps, max_det, max_tracks=max_tracks, iou_thre=0.3, max_age_us=2500, new_score_thre=0.25, class_agnostic=agnostic)
    full = tr.errors()
    assert full == tuple(int(v) for v in model.counters[:3]) and full[1:] == (0, 0)
    if max_tracks <= 5 and max_det >= 8:
        assert full[0] > 0                                                              # the table was full
    if max_tracks >= 64 and max_det == 100:
        assert int(model.next_id.max()) > 100 and int(model.hits.max()) >= 3


@gpu
def test_the_dense_sequence_needs_several_rounds_and_ties_go_by_index():
    """the sequences above need more than one mutual-best round (counted with the model's candidates), and a sequence of exact
    duplicates -- every IoU 1 or one of a few values, every decision a tie -- ends like the model"""
    steps = sequence(100, seed=64100)
    model = TM.TrackerModel(S, 100, max_tracks=64, iou_thre=0.3, max_age_us=2500, new_score_thre=0.25)
    most = 0
    for rec, counts, ends, due, reset in steps:
        for s in range(S):
            if due[s] and counts[s] > 0:
                r = rec[s].reshape(-1).view(BBOX_DTYPE)[:min(int(counts[s]), 100)]
                slots = [(i, model.box[s, i].copy(), model.cls[s, i]) for i in range(64) if model.ids[s, i]]
                dets = [(j, (r["x"][j], r["y"][j], r["w"][j], r["h"][j]), r["class_id"][j]) for j in range(len(r))]
                most = max(most, mutual_best_rounds(TM.candidates(slots, dets, 0.3, False))[1])
        model.step([rec[s].copy().reshape(-1).view(BBOX_DTYPE) for s in range(S)], counts, ends, due, reset)
    assert most >= 3
    dup = sequence(100, seed=7, duplicates=True)
    tr, model, out = run_both(dup, 100, max_tracks=64, iou_thre=0.3, max_age_us=2500, new_score_thre=0.25)
    ids = out[5][0].reshape(-1).view(BBOX_DTYPE)["track_id"][:int(dup[5][1][0])]
    assert len(ids) == 100 and (ids == 0).sum() > 0 and len(set(ids[ids != 0].tolist())) == (ids != 0).sum() and tr.errors()[0] > 0


@gpu
def test_clear_from_the_host_and_a_narrower_step():
    from sast_amd.tracking import DetectionTracker
    steps = sequence(8, seed=3, resets=False)
    tr, model = DetectionTracker(S, 100, max_tracks=5), TM.TrackerModel(S, 8, max_tracks=5)     # records narrower than the tracker's max_det
    for k, (rec, counts, ends, due, _reset) in enumerate(steps[:8]):
        if k == 4:
            tr.clear([1])
            model.reset_row(1)
        if k == 6:
            tr.clear()
            for s in range(S):
                model.reset_row(s)
            model.counters[:] = 0
        d_rec = _dev(rec)
        tr.step(d_rec, _dev(counts), _dev(ends), _dev(due.astype(bool)))
        want = rec.copy()
        model.step([want[s].reshape(-1).view(BBOX_DTYPE) for s in range(S)], counts, ends, due)
        assert np.array_equal(d_rec.cpu().numpy(), want), k
        assert_state(tr, model, k)


# ------------------------------------------------------------------------------------------------------------------ the recording driver

def _runs(steps, max_det):
    """per row the non-empty due steps as (t, records [m])"""
    rows = [[] for _ in range(S)]
    for rec, counts, ends, due, _reset in steps:
        for s in range(S):
            m = min(max(int(counts[s]), 0), max_det) if due[s] else 0
            if m:
                rows[s].append((int(ends[s]), rec[s, :m].copy()))
    return rows


@gpu
@pytest.mark.parametrize("max_tracks,max_det", [(64, 100), (5, 8), (128, 65)])
def test_track_recordings_equals_the_stepped_run(max_tracks, max_det):
    from sast_amd.tracking import DetectionTracker
    kw = dict(max_tracks=max_tracks, iou_thre=0.3, max_age_us=2500, new_score_thre=0.25)
    rows = _runs(sequence(max_det, seed=77 + max_det, resets=False), max_det)
    n = np.array([sum(len(r) for _t, r in row) for row in rows], np.int64)
    Dcap = int(n.max()) + 3
    log = np.random.RandomState(5).randint(0, 256, size=(S, Dcap, 40)).astype(np.uint8)     # records past n: random bytes
    for s, row in enumerate(rows):
        log[s, :n[s]] = np.concatenate([r for _t, r in row])
    # the stepped run: the rows' k-th runs side by side, a row that has none left is not due
    stepped, got_steps = DetectionTracker(S, max_det, **kw), [[] for _ in range(S)]
    for k in range(max(len(row) for row in rows)):
        rec, counts, ends, due = np.zeros((S, max_det, 40), np.uint8), np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S, np.uint8)
        for s, row in enumerate(rows):
            if k < len(row):
                t, r = row[k]
                rec[s, :len(r)], counts[s], ends[s], due[s] = r, len(r), t, 1
        d_rec = _dev(rec)
        stepped.step(d_rec, _dev(counts), _dev(ends), _dev(due))
        out = d_rec.cpu().numpy()
        for s in range(S):
            got_steps[s].append(out[s, :counts[s]])
    whole = DetectionTracker(S, max_det, **kw)
    d_log, d_n = _dev(log.view(np.int32).reshape(S, Dcap, 10)), _dev(n)
    first = np.zeros(S * max_det, BBOX_DTYPE)
    first["w"], first["h"], first["class_confidence"] = 4.0, 4.0, 1.0
    whole.step(_dev(first.view(np.uint8).reshape(S, max_det, 40)), _dev(np.ones(S, np.int32)), _dev(np.full(S, 5, np.int64)),
               _dev(np.ones(S, np.uint8)))                                               # a used table: the run starts from the reset state
    assert whole.ids[:, 0].tolist() == [1] * S
    whole.track_recordings(d_log, d_n)
    got = d_log.cpu().numpy().view(np.uint8).reshape(S, Dcap, 40)
    model = TM.TrackerModel(S, max_det, **kw)
    want = log.copy()
    model.run([want[s].reshape(-1).view(BBOX_DTYPE) for s in range(S)], n)
    assert np.array_equal(got, want)
    for s in range(S):
        assert np.array_equal(got[s, :n[s]], np.concatenate(got_steps[s])), s
    assert_state(whole, model, "run")
    for name in STATE:
        assert torch.equal(getattr(whole, name), getattr(stepped, name)), name
    assert whole.errors()[1:] == (0, 0) and int((got[:, :, 28:32].view(np.uint32) != log[:, :, 28:32].view(np.uint32)).sum()) > 10


@gpu
def test_track_recordings_cuts_long_runs_and_leaves_unsorted_rows():
    from sast_amd.tracking import DetectionTracker
    kw = dict(max_tracks=64, iou_thre=0.3, max_age_us=2500, new_score_thre=0.25)
    rows = _runs(sequence(100, seed=177, resets=False), 100)                             # runs of up to 100 records, a tracker for 8
    rows[1][3], rows[1][4] = (rows[1][4][0], rows[1][3][1]), (rows[1][3][0], rows[1][4][1])     # row 1: two runs swap their t
    n = np.array([sum(len(r) for _t, r in row) for row in rows], np.int64)
    Dcap = int(n.max())
    log = np.zeros((S, Dcap, 40), np.uint8)
    for s, row in enumerate(rows):
        for (t, r), at in zip(row, np.cumsum([0] + [len(r) for _t, r in row])):
            log[s, at:at + len(r)] = r
            log[s, at:at + len(r)].reshape(-1).view(BBOX_DTYPE)["t"] = t
    n[2] -= 30                                                                           # row 2 ends inside a run
    tr, model = DetectionTracker(S, 8, **kw), TM.TrackerModel(S, 8, **kw)
    d_log = _dev(log.view(np.int32).reshape(S, Dcap, 10))
    tr.track_recordings(d_log, _dev(n))
    want = log.copy()
    model.run([want[s].reshape(-1).view(BBOX_DTYPE) for s in range(S)], n)
    got = d_log.cpu().numpy().view(np.uint8).reshape(S, Dcap, 40)
    assert np.array_equal(got, want) and np.array_equal(got[1], log[1]) and np.array_equal(got[2, n[2]:], log[2, n[2]:])
    assert_state(tr, model, "cut")
    cut, unsorted = tr.errors()[1:]
    assert unsorted == 1 and cut == sum(len(r) > 8 for s in (0, 2) for _t, r in rows[s]) and cut > 10      # row 2's cut last run is still long
    lens = [len(r) for _t, r in rows[0]]
    at = int(np.sum(lens[:lens.index(100)]))                                             # a run of 100: ids on its first 8 only
    run = got[0].reshape(-1).view(BBOX_DTYPE)[at:at + 100]
    assert (run["t"] == run["t"][0]).all() and (run["track_id"][8:] == 0).all() and (run["track_id"][:8] != 0).any()
    tr.track_recordings(d_log, _dev(n))                                                  # the counters accumulate; the table starts over
    assert tr.errors()[1:] == (2 * cut, 2) and np.array_equal(d_log.cpu().numpy().view(np.uint8).reshape(S, Dcap, 40), want)


# ------------------------------------------------------------------------------------------------------------------ OnlineDetector

from test_online_detector import _chunk, _online, _push, _same, _session, _u8, detector  # noqa: E402,F401


def _with_model(model, od, got, reset):
    """what the model makes of the polled records of one push of a detector WITHOUT a tracker"""
    for s in range(S):
        if reset[s]:
            model.reset_row(s)
    ends, due = od.ends.cpu().numpy(), od.due.cpu().numpy()
    where = [(k, s) for k in range(od.W) for s in range(S) if due[k, s]]
    assert [s for _k, s in where] == [s for s, _a in got]
    out = []
    for (k, s), (_s, a) in zip(where, got):
        a = np.frombuffer(bytearray(a.tobytes()), BBOX_DTYPE)              # copied as bytes: a field-wise copy leaves the padding undefined
        assert (a["track_id"] == 0).all() and (a["t"] == ends[k, s]).all()
        model.step_row(s, a, ends[k, s])
        out.append((s, a))
    return out


@gpu
def test_online_detector_with_a_tracker_gives_the_plain_records_with_the_model_applied(detector):
    from sast_amd.tracking import DetectionTracker
    kw = dict(max_tracks=64, iou_thre=0.3, max_age_us=6000, new_score_thre=0.5)
    rounds, _recs, _e = _session(2, seed=41, reset_round=2, max_rounds=6)
    plain, tracked = _online(detector), _online(detector, tracker=DetectionTracker(S, 100, **kw))
    model = TM.TrackerModel(S, 100, **kw)
    ids, seen_again = 0, 0
    for parts, reset, final, *_m in rounds:
        _push(plain, parts, reset, final)
        _push(tracked, parts, reset, final)
        want = _with_model(model, plain, plain.drain(), reset)
        got = tracked.drain()
        _same(got, want)
        ids += sum(int((a["track_id"] != 0).sum()) for _s, a in got)
        seen_again = max(seen_again, int(model.hits.max()))
        assert_state(tracked.tracker, model, "push")
    print(f"online tracker: {ids} records with an id, longest track {seen_again} steps")
    assert ids > 0 and seen_again >= 2 and any(r[1].any() for r in rounds)
    assert tracked.errors() == plain.errors() and len(tracked.errors()) == 6


@gpu
def test_captured_push_with_a_tracker_and_a_log_replays_like_the_eager_run(detector):
    from sast_amd.online import DetectionLog
    from sast_amd.tracking import DetectionTracker
    kw = dict(max_tracks=64, iou_thre=0.3, max_age_us=6000, new_score_thre=0.5)
    rounds, _recs, _e = _session(2, seed=41, reset_round=2, max_rounds=4)
    eager = _online(detector, tracker=DetectionTracker(S, 100, **kw), log=DetectionLog(S, 4096))
    want = []
    for parts, reset, final, *_m in rounds:
        _push(eager, parts, reset, final)
        want.append(eager.drain())
    od = _online(detector, tracker=DetectionTracker(S, 100, **kw), log=DetectionLog(S, 4096))
    cols, counts = _chunk(rounds[0][0])
    reset, final = _u8(rounds[0][1]), _u8(rounds[0][2])
    od.push(*cols, counts, reset, final)
    _same(od.drain(), want[0])
    od.capture()
    for (parts, rst, fin, *_m), expect in zip(rounds[1:], want[1:]):
        new_cols, new_counts = _chunk(parts)
        for dst, src in zip(cols + [counts, reset, final], new_cols + [new_counts, _u8(rst), _u8(fin)]):
            dst.copy_(src)
        od.replay()
        _same(od.drain(), expect)
    for name in STATE:
        assert torch.equal(getattr(od.tracker, name), getattr(eager.tracker, name)), name
    assert torch.equal(od.log.records, eager.log.records) and torch.equal(od.log.counts, eager.log.counts)
    # the log holds the polled records, ids included, row by row in step order
    log, n = od.log.records.cpu().numpy().view(np.uint8).reshape(S, 4096, 40), od.log.counts.cpu().tolist()
    for s in range(S):
        flat = b"".join(a.tobytes() for step in want for row, a in step if row == s)      # as bytes: the padding of a record counts
        assert 40 * n[s] == len(flat) and log[s, :n[s]].tobytes() == flat, s
    assert sum(int((a["track_id"] != 0).sum()) for step in want for _s, a in step) > 0 and od.tracker.errors() == eager.tracker.errors()
