"""The tracker's rule without a GPU: tests/tracker_model.py against the definition (include/sast_hip.h, "track ids") on hand-written
cases, its invariants over seeded random sequences, the greedy order against the mutual-best rounds csrc/k_track.hip runs, and the host
contract of sast_tracker_step / sast_tracker_run and `DetectionTracker` (the library loaded, nothing launched)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_model as TM  # noqa: E402

from sast_amd.labels import BBOX_DTYPE  # noqa: E402


def recs(boxes, t=0, n=None):
    """[(x, y, w, h, class_id, confidence)] -> BBOX_DTYPE records with a canary track_id"""
    r = np.zeros(len(boxes) if n is None else n, BBOX_DTYPE)
    r["track_id"] = 0xABCD
    for j, b in enumerate(boxes):
        r[j]["x"], r[j]["y"], r[j]["w"], r[j]["h"], r[j]["class_id"], r[j]["class_confidence"] = b
        r[j]["t"] = t
    return r


def one(model, boxes, t, due=1, reset=None, count=None):
    r = recs(boxes, t)
    model.step([r], [len(boxes) if count is None else count], [t], [due], None if reset is None else [reset])
    return [int(v) for v in r["track_id"]]


def model(**kw):
    return TM.TrackerModel(1, kw.pop("max_det", 8), **{"max_tracks": 4, **kw})


A, B = (10.0, 10.0, 20.0, 20.0, 1, 0.9), (100.0, 50.0, 30.0, 10.0, 1, 0.8)


def moved(b, dx, dy=0.0):
    return (b[0] + dx, b[1] + dy) + tuple(b[2:])


# ------------------------------------------------------------------------------------------------------------------ the definition

def test_iou_is_the_fp32_formula_and_nan_is_no_candidate():
    a, b = np.array([0, 0, 3, 3], np.float32), np.array([1, 1, 3, 3], np.float32)
    assert TM.iou(a, b) == np.float32(np.float32(4) / np.float32(14)) and TM.iou(a, a) == 1 and TM.iou(a, a + np.float32([3, 0, 0, 0])) == 0
    assert TM.iou(a, np.float32([0, 0, 0, 0])) == 0 and TM.iou(np.float32([0, 0, 0, 0]), np.float32([0, 0, 0, 0])) == 0       # uni == 0
    for k in range(4):
        n = a.copy()
        n[k] = np.nan
        assert TM.iou(n, a) == 0 and TM.iou(a, n) == 0 and not TM.candidates([(0, n, 1)], [(0, a, 1)], 1e-6, False)
    assert TM.iou(np.float32([np.inf, 0, -np.inf, 3]), a) == 0                          # x2 = inf - inf


def test_a_box_that_drifts_keeps_its_id():
    m = model()
    assert one(m, [A, B], 1000) == [1, 2]
    for k in range(1, 6):
        assert one(m, [moved(B, 2.0 * k), moved(A, 1.5 * k)], 1000 + 50 * k) == [2, 1]
    assert m.ids[0].tolist() == [1, 2, 0, 0] and m.hits[0].tolist() == [6, 6, 0, 0] and m.last_t[0].tolist() == [1250, 1250, 0, 0]
    assert m.box[0, 0].tolist() == [17.5, 10.0, 20.0, 20.0] and m.next_id[0] == 3 and m.counters.tolist() == [0, 0, 0, 0]


def test_two_boxes_swap_by_iou_not_by_index():
    m = model()
    a, b = (0.0, 0.0, 10.0, 10.0, 1, 0.9), (6.0, 0.0, 10.0, 10.0, 1, 0.9)              # they overlap each other: IoU 4 / 16
    assert one(m, [a, b], 0) == [1, 2]
    assert one(m, [moved(b, 0.5), moved(a, 0.5)], 10) == [2, 1]                       # each detection overlaps both tracks
    # the order is global: detection 0 overlaps track 2 best (IoU 80 / 120) but detection 1 overlaps it better (90 / 110) and goes first;
    # detection 0 is left with track 1 (60 / 140).  Matching in index order would have given [2, 3]
    assert one(m, [moved(a, 4.5), moved(a, 7.5)], 20) == [1, 2]


def test_exact_ties_go_to_the_lower_detection_then_the_lower_slot():
    m = model()
    assert one(m, [A], 0) == [1]
    assert one(m, [A, A], 10) == [1, 2]                                               # one track, two identical detections
    assert one(m, [A], 20) == [1] and m.hits[0].tolist() == [3, 1, 0, 0]              # two identical slots, one detection: slot 0
    assert one(m, [A, A, A], 30) == [1, 2, 3]


def test_the_class_gate():
    other = A[:4] + (2, 0.9)
    m = model()
    assert one(m, [A], 0) == [1] and one(m, [other], 10) == [2] and m.cls[0].tolist() == [1, 2, 0, 0]
    m = model(class_agnostic=True)
    assert one(m, [A], 0) == [1] and one(m, [other], 10) == [1] and m.cls[0].tolist() == [1, 0, 0, 0]      # the slot keeps its class


def test_expiry_is_strictly_later_than_max_age_and_the_slot_is_reused_in_the_same_step():
    m = model(max_age_us=100)
    assert one(m, [A, B], 1000) == [1, 2]
    assert one(m, [B], 1050) == [2]                                                   # A's track was last seen at 1000
    assert one(m, [], 1100) == [] and m.ids[0].tolist() == [1, 2, 0, 0]               # 1100 - 1000 == max_age: kept
    far = (200.0, 200.0, 5.0, 5.0, 1, 0.9)
    assert one(m, [far], 1101) == [3]                                                 # one microsecond later: freed ...
    assert m.ids[0].tolist() == [3, 2, 0, 0] and m.hits[0].tolist() == [1, 2, 0, 0]   # ... and slot 0 taken by the birth
    assert one(m, [A], 50) == [4] and m.ids[0].tolist() == [3, 2, 4, 0]               # t went backwards: nothing expires


def test_a_full_table_gives_id_zero_and_counts():
    m = model(max_tracks=2)
    boxes = [(50.0 * k, 0.0, 10.0, 10.0, 1, 0.9) for k in range(4)]
    assert one(m, boxes, 0) == [1, 2, 0, 0] and m.counters.tolist() == [2, 0, 0, 0] and m.next_id[0] == 3
    assert one(m, boxes[::-1], 10) == [0, 0, 2, 1] and m.counters.tolist() == [4, 0, 0, 0]


def test_new_score_thre_and_a_nan_confidence():
    m = model(new_score_thre=0.5)
    lo, hi, nan = A[:5] + (0.49,), B[:5] + (0.5,), (300.0, 0.0, 5.0, 5.0, 1, np.nan)
    assert one(m, [lo, hi, nan], 0) == [0, 1, 0] and m.counters.tolist() == [0, 0, 0, 0]
    assert one(m, [B[:5] + (0.1,)], 10) == [1]                                        # the threshold is for births only


def test_a_nan_box_matches_nothing_and_is_born_as_it_is():
    m = model()
    bad = (np.nan,) + A[1:]
    assert one(m, [A], 0) == [1] and one(m, [bad, A], 10) == [2, 1]
    assert np.isnan(m.box[0, 1, 0]) and one(m, [bad, A], 20) == [3, 1]                # the NaN track is never continued


def test_due_zero_changes_nothing_and_reset_restarts_ids():
    m = model()
    assert one(m, [A, B], 0) == [1, 2]
    before = {k: v.copy() for k, v in m.state().items()}
    assert one(m, [A, B], 10 ** 9, due=0) == [0xABCD] * 2                             # not even expiry
    assert all(np.array_equal(before[k], v) for k, v in m.state().items())
    assert one(m, [A, B], 10, due=0, reset=1) == [0xABCD] * 2                         # the reset acts although the row is not due
    assert not m.ids.any() and not m.box.any() and not m.hits.any() and not m.last_t.any() and m.next_id[0] == 1
    assert one(m, [B, A], 20, reset=1) == [1, 2]
    assert one(m, [A, B], 30, count=1) == [2, 0xABCD]                                 # nothing at or past counts
    assert one(m, [A, B], 40, count=-3) == [0xABCD] * 2


def test_the_recording_driver_cuts_long_runs_and_refuses_unsorted_rows():
    m = TM.TrackerModel(2, 2, max_tracks=4)
    r0 = np.concatenate([recs([A, B, moved(B, 100.0)], 10), recs([B, A], 20)])
    r1 = np.concatenate([recs([A], 30), recs([A], 20), recs([A], 40)])
    r1 = np.concatenate([r1, recs([A], 5)])                                            # past n: not looked at
    m.run([r0, r1], [5, 3])
    assert r0["track_id"].tolist() == [1, 2, 0, 2, 1] and r1["track_id"].tolist() == [0xABCD] * 4
    assert m.counters.tolist() == [0, 1, 1, 0] and not m.ids[1].any() and m.ids[0].tolist() == [1, 2, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ properties

def _random_steps(rng, steps, max_det, classes=2):
    live, out = [], []
    for _ in range(steps):
        live = [(x + rng.randint(-4, 5) * 0.25, y + rng.randint(-4, 5) * 0.25, w, h, c) for x, y, w, h, c in live if rng.rand() > 0.15]
        for _b in range(rng.randint(0, 4)):
            live.append((rng.randint(0, 160) * 0.25, rng.randint(0, 160) * 0.25, rng.randint(4, 80) * 0.25, rng.randint(4, 80) * 0.25,
                         rng.randint(classes)))
        boxes = [b + (rng.randint(1, 100) / 100.0,) for b in live]
        rng.shuffle(boxes)
        out.append(boxes[:max_det])
    return out


@pytest.mark.parametrize("seed", range(4))
def test_ids_are_unique_between_resets_and_a_matched_id_was_live_before_the_step(seed):
    rng = np.random.RandomState(seed)
    m = TM.TrackerModel(1, 12, max_tracks=[3, 6, 16, 16][seed], iou_thre=0.3, max_age_us=[100, 150, 150, 10 ** 6][seed], new_score_thre=0.2,
                        class_agnostic=bool(seed & 1))
    born, top, matched = set(), 0, 0
    for k, boxes in enumerate(_random_steps(rng, 60, 12)):
        reset = int(k in (20, 41))
        if reset:
            born, top = set(), 0
        r = recs(boxes, 100 * k)
        if reset:
            m.reset_row(0)
        live_before, match = m.step_row(0, r, 100 * k)
        ids = [int(v) for v in r["track_id"]]
        assert len([v for v in ids if v]) == len({v for v in ids if v})                  # no id twice in a step
        for j, v in enumerate(ids):
            if j in match:
                assert v in live_before and v in born
                matched += 1
            elif v:
                assert v == top + 1 and v not in born                                    # births count up from 1, in index order
                top = v
                born.add(v)
        live = m.ids[0][m.ids[0] != 0].tolist()
        assert len(live) == len(set(live)) and set(live) <= born and int(m.next_id[0]) == top + 1
    assert matched > 40


def mutual_best_rounds(cands):
    """what the kernel runs: every slot and every detection pick their best remaining candidate in the strict order, the pairs that
    chose each other are fixed, repeat -> ({j: i}, rounds)"""
    order = lambda c: (-float(c[0]), c[1], c[2])  # noqa: E731
    left, match, rounds = list(cands), {}, 0
    while left:
        rounds += 1
        by_slot, by_det = {}, {}
        for c in left:
            if c[2] not in by_slot or order(c) < order(by_slot[c[2]]):
                by_slot[c[2]] = c
            if c[1] not in by_det or order(c) < order(by_det[c[1]]):
                by_det[c[1]] = c
        fixed = [c for c in by_slot.values() if by_det[c[1]] is c]
        assert fixed
        for _v, j, i in fixed:
            match[j] = i
        left = [c for c in left if c[1] not in match and c[2] not in match.values()]
    return match, rounds


@pytest.mark.parametrize("seed", range(6))
def test_greedy_over_the_sorted_list_equals_the_mutual_best_rounds(seed):
    rng = np.random.RandomState(40 + seed)
    most = 0
    for _ in range(40):
        n_s, n_d = rng.randint(1, 20), rng.randint(1, 20)
        if seed < 3:                                                                      # few distinct values: ties everywhere
            vals = rng.randint(1, 4, size=(n_s, n_d)).astype(np.float32) / 4
        else:
            vals = rng.rand(n_s, n_d).astype(np.float32)
        cands = [(vals[i, j], j, i) for i in range(n_s) for j in range(n_d) if rng.rand() < 0.7]
        got, rounds = mutual_best_rounds(cands)
        assert got == TM.greedy(cands)
        most = max(most, rounds)
    assert most >= 3                                                                      # the chains that need several rounds occur


# ------------------------------------------------------------------------------------------------------------------ the host contract

def test_tracker_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_tracker_")]
    assert names == ["sast_tracker_run", "sast_tracker_step"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n)
    P = C.c_void_p
    assert _lib._SIGNATURES["sast_tracker_step"] == (C.c_int, [C.POINTER(_lib.SastTrackerArgs), C.POINTER(_lib.SastTrackStepArgs), P])
    assert _lib._SIGNATURES["sast_tracker_run"] == (C.c_int, [C.POINTER(_lib.SastTrackerArgs), C.POINTER(_lib.SastTrackRunArgs), P])
    assert (_lib.TRACK_MAX_TRACKS, _lib.TRACK_MAX_DET, _lib.TRACK_MAX_PAIRS) == (128, 1792, 65536)
    assert 32 * _lib.TRACK_MAX_DET + 40 * _lib.TRACK_MAX_TRACKS + 64 <= 64 * 1024           # the LDS plan fits the default 64 KiB


def _args(_lib, **kw):
    q = 0x1000
    tr = dict(ids=q, box=q, cls=q, last_t=q, hits=q, next_id=q, counters=q, S=3, max_tracks=64, max_det=100, class_agnostic=0, iou_thre=0.3,
              new_score_thre=0.0, max_age_us=200000)
    st = dict(records=q, counts=q, ends=q, due=q, reset=q)
    ru = dict(records=q, n=q, Dcap=1000)
    out = []
    for cls, d in ((_lib.SastTrackerArgs, tr), (_lib.SastTrackStepArgs, st), (_lib.SastTrackRunArgs, ru)):
        a = cls()
        for k, v in d.items():
            setattr(a, k, kw.get(cls.__name__ + "." + k, v if k == "records" else kw.get(k, v)))     # `records` is named per struct
        out.append(a)
    return out


def test_tracker_rejects_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()

    # every call below is refused: one that passed the checks would launch a kernel on these made-up addresses
    def step(**kw):
        tr, st, _ru = _args(_lib, **kw)
        return lib.sast_tracker_step(C.byref(tr), C.byref(st), None)

    def run(**kw):
        tr, _st, ru = _args(_lib, **kw)
        return lib.sast_tracker_run(C.byref(tr), C.byref(ru), None)

    def both(**kw):
        return step(**kw), run(**kw)

    for name in ("ids", "box", "cls", "last_t", "hits", "next_id", "counters"):
        assert both(**{name: None}) == (-22, -22), name
    for kw in (dict(S=0), dict(S=65536), dict(max_tracks=0), dict(max_tracks=129), dict(max_det=0), dict(max_det=-1), dict(max_det=1793),
               dict(max_tracks=128, max_det=513), dict(max_tracks=65, max_det=1009), dict(iou_thre=0.0), dict(iou_thre=-0.5),
               dict(iou_thre=1.0000001), dict(iou_thre=float("nan")), dict(new_score_thre=float("nan")), dict(max_age_us=-1)):
        assert both(**kw) == (-22, -22), kw
    for name in ("counts", "ends", "due"):
        assert step(**{name: None}) == -22, name
    assert run(n=None) == -22
    assert step(**{"SastTrackStepArgs.records": None}) == -22 and run(**{"SastTrackRunArgs.records": None}) == -22
    assert step(**{"SastTrackStepArgs.records": 0x1004}) == -22 and run(**{"SastTrackRunArgs.records": 0x1004}) == -22
    for kw in (dict(Dcap=0), dict(Dcap=-5), dict(S=3, Dcap=(2 ** 31 - 1) // 3 + 1), dict(S=1, Dcap=2 ** 31)):
        assert run(**kw) == -22, kw
    tr, st, ru = _args(_lib)
    assert lib.sast_tracker_step(None, C.byref(st), None) == -22 and lib.sast_tracker_step(C.byref(tr), None, None) == -22
    assert lib.sast_tracker_run(None, C.byref(ru), None) == -22 and lib.sast_tracker_run(C.byref(tr), None, None) == -22


def test_detection_tracker_python_argument_validation():
    from sast_amd.tracking import DetectionTracker
    for kw, match in ((dict(num_streams=0), "num_streams"), (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=129), "max_tracks"),
                      (dict(max_det=0), "max_det"), (dict(max_det=1793), "max_det"), (dict(max_det=513, max_tracks=128), "max_det"),
                      (dict(iou_thre=0.0), "iou_thre"), (dict(iou_thre=1.5), "iou_thre"), (dict(new_score_thre=float("nan")), "NaN"),
                      (dict(max_age_us=-1), "max_age_us")):
        with pytest.raises(ValueError, match=match):
            DetectionTracker(**{"num_streams": 3, "max_det": 8, **kw})
    tr = DetectionTracker(3, 8)
    assert tr.errors() == (0, 0, 0)
    tr.clear()
    rec, cnt, ends, due = torch.zeros(3, 8, 40, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.ones(3, dtype=torch.uint8)
    for bad in (dict(records=torch.zeros(2, 8, 40, dtype=torch.uint8)), dict(records=torch.zeros(3, 9, 40, dtype=torch.uint8)),
                dict(records=torch.zeros(3, 8, 10, dtype=torch.int32)), dict(counts=cnt.long()), dict(ends=ends.int()), dict(due=None),
                dict(due=torch.ones(2, dtype=torch.uint8)), dict(reset=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises((ValueError, TypeError), match="sast_amd.tracking"):
            tr.step(**{**dict(records=rec, counts=cnt, ends=ends, due=due), **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.step(rec, cnt, ends, due)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.step(rec[:, :5].contiguous(), cnt, ends, due.bool(), torch.zeros(3, dtype=torch.bool))
    log = torch.zeros(3, 50, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="sast_amd.tracking"):
        tr.track_recordings(log, cnt)
    with pytest.raises(ValueError, match="sast_amd.tracking"):
        tr.track_recordings(log.view(3, 50 * 10), ends)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.track_recordings(log, ends)
    assert tr.ids is None                                                                # nothing was allocated on the way


def test_online_detector_refuses_a_tracker_for_other_streams_or_fewer_records():
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    from sast_amd.tracking import DetectionTracker

    class _Det:
        training = False

        class yolox_head:
            num_classes = 2

    def queue():
        return EventQueue(3, 8192, duration_us=600, height=128, width=160)

    for bad in (DetectionTracker(2, 100), DetectionTracker(3, 99), object()):
        with pytest.raises(ValueError, match="tracker must be a DetectionTracker"):
            OnlineDetector(_Det(), queue(), windows_per_step=2, max_det=100, tracker=bad)
    od = OnlineDetector(_Det(), queue(), windows_per_step=2, max_det=100, tracker=DetectionTracker(3, 128))
    assert od.tracker.max_det == 128 and OnlineDetector(_Det(), queue(), windows_per_step=2).tracker is None
    cols = [torch.zeros(3, 8, dtype=torch.int64) for _ in range(4)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        od.push(*cols, torch.zeros(3, dtype=torch.int64))
