"""sast_amd.tracking.TrackingEvaluator on the MI355X against the sequential model (tests/tracking_eval_model.py): every integer of
`te.rows` and of the accumulator equal, the fp64 IoU sums within 1e-12 relative (the bar of the evaluator's six numbers), on the
recordings of tests/tracking_eval_cases.py.  tests/test_tracking_eval_model.py checks on the CPU that every frame of them has a unique
optimal assignment (margin >= 1e-5), so the device solver, which sums in another order than scipy, has to find the same matching, and
that in the crowded ones a greedy matching gives other counts.  Frames of 0, 1, 63, 64, 65 and 128 labels and hypotheses in both
rectangular directions, an empty recording and one of a single frame, class_agnostic on and off, an off-grid detector clock; then the
refusals, a perfect tracker, `DetectionTracker.track_recordings` end to end, graph capture and `merge`."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_eval_cases as CS  # noqa: E402
import tracking_eval_model as M  # noqa: E402

from sast_amd.labels import BBOX_DTYPE  # noqa: E402

gpu = pytest.mark.gpu
REL = 1e-12


@functools.lru_cache(maxsize=None)
def scenarios():
    return CS.scenarios()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def model_of(kw, recordings, calls=1):
    """the model fed the recordings `calls` times -> (model, rows, iou, diag of the last call)"""
    m = M.TrackingEvalModel(2, 900.0, 10.0, diagnose=False, **kw)
    for _ in range(calls):
        rows, iou, diag, _frames = m.add_recordings([g for g, _d in recordings], [d for _g, d in recordings])
    return m, rows, iou, diag


def evaluator(kw):
    from sast_amd.tracking import TrackingEvaluator
    return TrackingEvaluator("gen1", False, **kw)


def assert_rows(te, rows, iou, where):
    got_rows, got_iou = (t.cpu().numpy() for t in te.rows)
    assert got_rows.dtype == np.int64 and got_rows.shape == rows.shape and got_iou.dtype == np.float64 and got_iou.shape == iou.shape
    print(f"{where}: rows\n{got_rows[:, -1]}\nlargest IoU-sum difference {np.abs(got_iou - iou).max():.3g} of {np.abs(iou).max():.6g}")
    assert np.array_equal(got_rows, rows), where
    assert (np.abs(got_iou - iou) <= REL * np.abs(iou)).all(), where


def assert_accumulator(te, m, where):
    counts, iou, diag = te._numbers()
    assert np.array_equal(counts, m.acc) and np.array_equal(diag, m.acc_diag), where
    assert (np.abs(iou - m.acc_iou) <= REL * np.abs(m.acc_iou)).all(), where
    assert te.errors() == dict(zip(M.DIAG, m.acc_diag.tolist())), where


def assert_evaluate(te, m):
    got, want = te.evaluate(), m.evaluate()
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, int):
            assert got[k] == v and isinstance(got[k], int), k
        else:
            assert (np.isnan(v) and np.isnan(got[k])) or abs(got[k] - v) <= 1e-12 * abs(v), k
    per = te.per_class()
    for k, name in enumerate(te.classes):
        assert {c: per[name][c] for c in M.COLS} == {c: m.evaluate(k)[c] for c in M.COLS}, name


# ------------------------------------------------------------------------------------------------------------------ against the model

@gpu
@pytest.mark.parametrize("name", ["edge", "edge_agnostic_tol", "crowd_grid", "crowd", "grid_half"])
def test_rows_and_accumulator_equal_the_model(name):
    kw, recordings = scenarios()[name]
    m, rows, iou, _diag = model_of(kw, recordings, calls=2)
    te = evaluator(kw)
    tensors = [_dev(a) for a in CS.packed(recordings)]
    te.add_recordings(*tensors)
    assert_rows(te, rows, iou, name)
    te.add_recordings(*tensors)
    assert_rows(te, rows, iou, name + ", second call")
    assert_accumulator(te, m, name)
    assert_evaluate(te, m)
    assert te.evaluate()["matches"] > 1000 and te.evaluate()["idsw"] > 0 and te.evaluate()["frag"] > 0
    te.reset()
    assert te.evaluate()["gt"] == 0 and not any(te.errors().values())
    te.add_recordings(*tensors)
    assert te._numbers()[0].tolist() == rows.sum(axis=0).tolist()                         # one call's rows, and nothing from before the reset


@gpu
def test_a_table_filled_to_exactly_max_gt_tracks_and_one_id_more():
    kw, recordings = scenarios()["edge"]
    full = dict(kw, max_gt_tracks=128)                                                    # the first recording has 128 labelled tracks
    m, rows, iou, _diag = model_of(full, recordings)
    assert int(rows[0, 2, M.C["gt_tracks"]]) == 128
    te = evaluator(full)
    tensors = [_dev(a) for a in CS.packed(recordings)]
    te.add_recordings(*tensors)
    assert_rows(te, rows, iou, "max_gt_tracks = 128")
    assert_evaluate(te, m)
    over = dict(kw, max_gt_tracks=127)
    m, rows, iou, _diag = model_of(over, recordings)
    assert not rows[0].any() and rows[2].any()
    te = evaluator(over)
    te.add_recordings(*tensors)
    assert_rows(te, rows, iou, "max_gt_tracks = 127")
    assert_accumulator(te, m, "max_gt_tracks = 127")
    assert te.errors()["refused_tracks"] == 1
    with pytest.raises(OverflowError, match="1 recording.s. refused for max_gt_tracks=127"):
        te.evaluate()


@gpu
@pytest.mark.parametrize("limit,word", [("max_labels_per_frame", "refused_labels"), ("max_hyp_per_frame", "refused_hyp")])
def test_a_frame_one_over_a_limit_refuses_its_row_alone(limit, word):
    kw, recordings = scenarios()["edge"]
    kw = dict(kw, **{limit: 127})                                                         # the first recording has frames of 128
    m, rows, iou, _diag = model_of(kw, recordings)
    assert not rows[0].any() and rows[2].any()
    te = evaluator(kw)
    te.add_recordings(*[_dev(a) for a in CS.packed(recordings)])
    assert_rows(te, rows, iou, limit)
    assert_accumulator(te, m, limit)
    assert te.errors()[word] == 1 and sum(te.errors().values()) == sum(m.acc_diag)
    with pytest.raises(OverflowError, match=limit + "=127"):
        te.per_class()


@gpu
@pytest.mark.parametrize("side", ["labels", "detections"])
def test_an_unsorted_row_adds_nothing_and_evaluate_raises(side):
    kw, recordings = scenarios()["grid_half"]
    recordings = [tuple(a.copy() for a in r) for r in recordings]
    a = recordings[1][0 if side == "labels" else 1]
    i = len(a) // 2
    a["t"][i] = a["t"][i - 1] - 1
    m, rows, iou, _diag = model_of(kw, recordings)
    assert not rows[1].any() and rows[0].any() and rows[2].any() and m.acc_diag.tolist()[0] == 1
    te = evaluator(kw)
    te.add_recordings(*[_dev(x) for x in CS.packed(recordings)])
    assert_rows(te, rows, iou, side)
    assert_accumulator(te, m, side)
    with pytest.raises(ValueError, match="1 recording.s. given to add_recordings were not sorted"):
        te.evaluate()


# ------------------------------------------------------------------------------------------------------------------ with the tracker

@gpu
def test_a_perfect_tracker_has_mota_one():
    kw, perfect = CS.perfect_case()
    m, rows, iou, _diag = model_of(kw, perfect)
    te = evaluator(kw)
    te.add_recordings(*[_dev(a) for a in CS.packed(perfect)])
    assert_rows(te, rows, iou, "perfect")
    e = te.evaluate()
    assert e["MOTA"] == 1.0 and abs(e["MOTP"] - 1.0) < 1e-6 and e["recall"] == 1.0 and e["precision"] == 1.0
    assert (e["idsw"], e["frag"], e["fp"], e["fn"], e["pt"], e["ml"]) == (0, 0, 0, 0, 0, 0) and e["matches"] == e["gt"] == e["hyp"] > 1000
    assert e["mt"] == e["gt_tracks"] > 100


@gpu
def test_track_recordings_scored_on_the_device_equals_the_model_on_the_same_records():
    from sast_amd.tracking import DetectionTracker
    kw, recordings = CS.untracked_case()
    gt, n_gt, dt, n_dt = (_dev(a) for a in CS.packed(recordings))
    tracker = DetectionTracker(len(recordings), CS.TRACKER_MAX_DET, **CS.TRACKER)
    tracker.track_recordings(dt, n_dt)
    te = evaluator(kw)
    te.add_recordings(gt, n_gt, dt, n_dt)                                                 # the tracker's tensor goes in as it is
    assert tracker.errors() == (0, 0, 0)
    got = dt.cpu().numpy().view(np.uint8).reshape(len(recordings), -1, 40)
    tracked = [(g, np.frombuffer(got[s, :len(d)].tobytes(), BBOX_DTYPE)) for s, (g, d) in enumerate(recordings)]
    want = CS.tracked_by_the_model(recordings)                                            # the records the CPU test checked the margins of
    for (_g, a), (_g2, b) in zip(tracked, want):
        assert all(np.array_equal(a[f], b[f]) for f in BBOX_DTYPE.names)
    m, rows, iou, _diag = model_of(kw, tracked)
    assert_rows(te, rows, iou, "tracked")
    assert_evaluate(te, m)
    e = te.evaluate()
    print("the greedy tracker on jittered copies of the labels:", e)
    assert e["matches"] > 1000 and e["MOTA"] > 0.5 and e["mt"] > 100


# ------------------------------------------------------------------------------------------------------------------ capture and merge

@gpu
def test_a_captured_add_replays_on_new_records_like_the_eager_call():
    kw, first = scenarios()["grid_half"]
    kw2, second = scenarios()["edge"]
    assert kw == kw2
    caps = tuple(max(len(r[side]) for r in first + second) + 2 for side in (0, 1))
    a, b = CS.packed(first, caps), CS.packed(second, caps)
    tensors = [_dev(x) for x in a]
    te = evaluator(kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        te.add_recordings(*tensors)                                                       # the eager call: it allocates
    torch.cuda.current_stream().wait_stream(side)
    te.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                             # would fail on any synchronisation or allocation
        te.add_recordings(*tensors)
    te.reset()
    m = M.TrackingEvalModel(2, 900.0, 10.0, diagnose=False, **kw)
    for data, recordings in ((b, second), (a, first)):
        for dst, src in zip(tensors, data):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        g.replay()
        rows, iou, _diag, _frames = m.add_recordings([x for x, _d in recordings], [d for _x, d in recordings])
        assert_rows(te, rows, iou, "replay")
    assert_accumulator(te, m, "two replays")
    eager = evaluator(kw)
    for data in (b, a):
        eager.add_recordings(*[_dev(x) for x in data])
    assert torch.equal(eager._acc, te._acc)                                               # the same bits, the IoU sums included


@gpu
def test_merge_equals_one_evaluator_fed_both():
    kw, first = scenarios()["crowd_grid"]
    second = first[::-1]
    one, two, both = evaluator(kw), evaluator(kw), evaluator(kw)
    ta, tb = [_dev(x) for x in CS.packed(first)], [_dev(x) for x in CS.packed(second)]
    one.add_recordings(*ta)
    two.add_recordings(*tb)
    both.add_recordings(*ta)
    both.add_recordings(*tb)
    one.merge(two)
    counts, iou, diag = one._numbers()
    want_counts, want_iou, want_diag = both._numbers()
    assert np.array_equal(counts, want_counts) and np.array_equal(diag, want_diag) and counts[2, 3] > 2000
    assert (np.abs(iou - want_iou) <= REL * np.abs(want_iou)).all()
    assert one.evaluate()["matches"] == both.evaluate()["matches"] and one.per_class().keys() == both.per_class().keys()
    empty = evaluator(kw)
    empty.merge(one)                                                                      # into an evaluator that has not been used
    assert empty.evaluate() == one.evaluate()
