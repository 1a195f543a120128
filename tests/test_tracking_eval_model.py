"""The tracking evaluator's rule on the CPU (tests/tracking_eval_model.py): hand-worked recordings with every count written out, the
scipy assignment against a brute force, and the conditions the GPU test's recordings (tests/tracking_eval_cases.py) must meet -- a
unique optimum in every frame, frames where the optimal matching is not the greedy one, frames where the carry-over decides.  Then the
argument checks of `TrackingEvaluator`, which need no GPU."""
import itertools
import math
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

T = [600_000 + 50_000 * i for i in range(8)]


def recs(*rows):
    """(t, x, y, w, h, class_id, track_id) per record"""
    out = np.zeros(len(rows), BBOX_DTYPE)
    for i, (t, x, y, w, h, c, tid) in enumerate(rows):
        out[i] = (t, x, y, w, h, c, tid, 0.5)
    return out


def model(**kw):
    return M.TrackingEvalModel(2, 900.0, 10.0, **kw)          # gen1: two classes, diag 30, side 10


def counts(r, k=2):
    return {name: int(r["rows"][k, i]) for i, name in enumerate(M.COLS)}


def expect(r, k=2, **want):
    base = dict.fromkeys(M.COLS, 0)
    base.update(want)
    assert counts(r, k) == base


# ------------------------------------------------------------------------------------------------------------------ hand-worked recordings

def test_an_identity_switch():
    gt = recs(*[(T[i], 50, 50, 40, 40, 0, 1) for i in range(3)])
    dt = recs((T[0], 50, 50, 40, 40, 0, 5), (T[1], 50, 50, 40, 40, 0, 5), (T[2], 50, 50, 40, 40, 0, 6))
    r = model().recording(gt, dt)
    expect(r, frames=3, gt=3, hyp=3, matches=3, idsw=1, gt_tracks=1, mt=1)
    expect(r, k=0, frames=3, gt=3, hyp=3, matches=3, idsw=1, gt_tracks=1, mt=1)
    expect(r, k=1, frames=3)
    assert r["iou"].tolist() == [3.0, 0.0, 3.0]


def test_a_fragmentation_and_a_partially_tracked_track():
    gt = recs(*[(T[i], 50, 50, 40, 40, 1, 9) for i in range(4)])
    dt = recs((T[0], 50, 50, 40, 40, 1, 5), (T[1], 50, 50, 40, 40, 1, 5), (T[3], 50, 50, 40, 40, 1, 5))
    r = model().recording(gt, dt)
    expect(r, frames=4, gt=4, hyp=3, matches=3, fn=1, frag=1, gt_tracks=1, pt=1)          # 5 * 3 < 4 * 4: not mostly tracked
    expect(r, k=1, frames=4, gt=4, hyp=3, matches=3, fn=1, frag=1, gt_tracks=1, pt=1)


def test_a_track_lost_for_good_and_the_thresholds_of_the_track_classes():
    gt = recs(*[(T[i], 50, 50, 40, 40, 0, 1) for i in range(5)], *[(T[i], 150, 50, 40, 40, 0, 2) for i in range(5)])
    gt = gt[np.argsort(gt["t"], kind="stable")]
    # track 1 never has a hypothesis near it; track 2 has one in 1 of 5 frames (5 * 1 < 5 is false: partially tracked), the hypothesis
    # next to track 1 overlaps it by a third only
    dt = recs(*[(T[i], 76, 50, 40, 40, 0, 3) for i in range(5)], (T[2], 150, 50, 40, 40, 0, 4))
    dt = dt[np.argsort(dt["t"], kind="stable")]
    r = model().recording(gt, dt)
    expect(r, frames=5, gt=10, hyp=6, matches=1, fp=5, fn=9, gt_tracks=2, ml=1, pt=1)
    four = model().recording(recs(*[(T[i], 50, 50, 40, 40, 0, 1) for i in range(5)]), recs(*[(T[i], 50, 50, 40, 40, 0, 3) for i in range(4)]))
    expect(four, frames=5, gt=5, hyp=4, matches=4, fn=1, gt_tracks=1, mt=1)               # 5 * 4 >= 4 * 5: mostly tracked


def test_the_carry_over_keeps_a_pair_the_assignment_alone_would_swap():
    # frame 2: A at x = 0 and B at x = 10; hypothesis 5 (A's) at x = 8 and 6 (B's) at x = 2: IoU 32 / 48 with the own track, 38 / 42
    # with the other one.  The assignment alone takes the crossed pairs and counts two identity switches.
    gt = recs((T[0], 0, 0, 40, 40, 0, 1), (T[0], 100, 0, 40, 40, 0, 2), (T[1], 0, 0, 40, 40, 0, 1), (T[1], 10, 0, 40, 40, 0, 2))
    dt = recs((T[0], 0, 0, 40, 40, 0, 5), (T[0], 100, 0, 40, 40, 0, 6), (T[1], 8, 0, 40, 40, 0, 5), (T[1], 2, 0, 40, 40, 0, 6))
    m = model()
    r = m.recording(gt, dt)
    expect(r, frames=2, gt=4, hyp=4, matches=4, gt_tracks=2, mt=2)
    assert [f["carry_changes"] for f in r["frames"]] == [False, True]
    assert r["iou"][2] == 2.0 + 2.0 * float(np.float32(32.0) / np.float32(48.0))
    lab, hyp = gt[2:], dt[2:]
    v, ok = m._pairs(lab, hyp)
    assert m._match(lab, hyp, {}, v, ok)[0] == {0: 1, 1: 0} and m._match(lab, hyp, {1: 5, 2: 6}, v, ok)[0] == {0: 0, 1: 1}


@pytest.mark.parametrize("first", ["A", "B"])
def test_two_labels_whose_last_hypothesis_is_the_same_id(first):
    a, b = (50, 50, 40, 40, 0, 1), (54, 50, 40, 40, 1, 2)                                 # A is a car, B a pedestrian
    both = [(T[2],) + a, (T[2],) + b] if first == "A" else [(T[2],) + b, (T[2],) + a]
    gt = recs((T[0],) + a, (T[1],) + b, *both)
    dt = recs(*[(T[i], 52, 50, 40, 40, 0, 5) for i in range(3)])
    r = model(class_agnostic=True).recording(gt, dt)                                      # both tracks end frames 1 and 2 with last = 5
    expect(r, frames=3, gt=4, hyp=3, matches=3, fn=1, gt_tracks=2, pt=1, mt=1)
    won, lost = (0, 1) if first == "A" else (1, 0)                                        # the earlier record keeps the hypothesis
    expect(r, k=won, frames=3, gt=2, matches=2, gt_tracks=1, mt=1, hyp=3 if won == 0 else 0)
    expect(r, k=lost, frames=3, gt=2, matches=1, fn=1, gt_tracks=1, pt=1, hyp=3 if lost == 0 else 0)


def test_a_frame_with_no_run_inside_the_tolerance_and_the_nearest_run():
    gt = recs((T[0], 50, 50, 40, 40, 0, 1), (T[1], 50, 50, 40, 40, 0, 1), (T[2], 50, 50, 40, 40, 0, 1))
    # frame 0: a run 1001 us late; frame 1: runs 400 us before and after (the earlier one is taken: it holds id 5), frame 2: 1000 us early
    dt = recs((T[0] + 1001, 50, 50, 40, 40, 0, 5), (T[1] - 400, 50, 50, 40, 40, 0, 5), (T[1] + 400, 50, 50, 40, 40, 0, 6),
              (T[2] - 1000, 50, 50, 40, 40, 0, 5))
    r = model(time_tol_us=1000).recording(gt, dt)
    expect(r, frames=3, gt=3, hyp=2, matches=2, fn=1, gt_tracks=1, pt=1)
    exact = model(time_tol_us=0).recording(gt, dt)
    expect(exact, frames=3, gt=3, fn=3, gt_tracks=1, ml=1)


def test_duplicates_and_track_id_zero_and_foreign_classes_are_dropped_and_counted():
    gt = recs((T[0], 50, 50, 40, 40, 0, 1), (T[0], 150, 50, 40, 40, 0, 1),               # a second record of track 1: dropped
              (T[0], 250, 50, 40, 40, 2, 3),                                              # class 2 of a two-class dataset
              (T[0], 350, 50, 40, 5, 0, 4),                                               # too flat for the filter: not counted anywhere
              (400_000, 50, 50, 40, 40, 0, 8))                                            # before 0.5 s
    gt = gt[np.argsort(gt["t"], kind="stable")]
    dt = recs((T[0], 300, 300, 40, 40, 0, 5), (T[0], 50, 50, 40, 40, 0, 5),              # the first record of id 5 is far away and stays
              (T[0], 50, 50, 40, 40, 0, 0),                                               # untracked
              (T[0], 50, 50, 40, 40, 3, 6))
    r = model().recording(gt, dt)
    expect(r, frames=1, gt=1, hyp=1, fp=1, fn=1, gt_tracks=1, ml=1)
    assert dict(zip(M.DIAG, r["diag"].tolist())) == dict(unsorted=0, refused_labels=0, refused_hyp=0, refused_tracks=0, untracked=1,
                                                         bad_class=2, duplicate_labels=1, duplicate_hyp=1)


def test_refusals_and_the_unsorted_row_add_nothing():
    gt = recs(*[(T[0], 50 * i, 50, 40, 40, 0, i + 1) for i in range(3)], (T[1], 0, 50, 40, 40, 0, 9))
    dt = recs(*[(T[0], 50 * i, 50, 40, 40, 0, i + 1) for i in range(3)])
    for kw, why in ((dict(max_labels_per_frame=2), "refused_labels"), (dict(max_hyp_per_frame=2), "refused_hyp"), (dict(max_gt_tracks=3), "refused_tracks")):
        r = model(**kw).recording(gt, dt)
        assert not r["rows"].any() and not r["iou"].any() and dict(zip(M.DIAG, r["diag"].tolist()))[why] == 1 and r["diag"].sum() == 1
    expect(model(max_labels_per_frame=3, max_hyp_per_frame=3, max_gt_tracks=4).recording(gt, dt), frames=2, gt=4, hyp=3, matches=3, fn=1,
           gt_tracks=4, mt=3, ml=1)
    r = model().recording(gt[::-1], dt)
    assert not r["rows"].any() and r["diag"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_the_derived_floats():
    m = model()
    e = m.evaluate()
    assert all(math.isnan(e[k]) for k in ("MOTA", "MOTP", "recall", "precision"))
    m.add_recordings([recs((T[0], 50, 50, 40, 40, 0, 1), (T[0], 150, 50, 40, 40, 0, 2))], [recs((T[0], 50, 50, 40, 30, 0, 5), (T[0], 300, 50, 40, 40, 0, 6))])
    e = m.evaluate()
    assert (e["gt"], e["matches"], e["fp"], e["fn"], e["idsw"]) == (2, 1, 1, 1, 0)
    assert e["MOTA"] == 1.0 - 2 / 2 and e["MOTP"] == float(np.float32(1200.0) / np.float32(1600.0)) and e["recall"] == 0.5 and e["precision"] == 0.5
    assert math.isnan(m.evaluate(1)["MOTA"]) and m.evaluate(0)["gt"] == 2


# ------------------------------------------------------------------------------------------------------------------ the solver

def brute(cost, ok):
    """every matching of rows to columns: the most valid pairs, then the least cost sum -> (pairs, cost, the runner-up's cost)"""
    n, m = ok.shape
    best = []
    small, big, by_row = (n, m, True) if n <= m else (m, n, False)
    seen = {}
    for perm in itertools.permutations(range(big), small):
        pairs = tuple(sorted((r, c) if by_row else (c, r) for r, c in enumerate(perm) if (ok[r, c] if by_row else ok[c, r])))
        seen[pairs] = sum(cost[r, c] for r, c in pairs)
    most = max(len(p) for p in seen)
    best = sorted((v, p) for p, v in seen.items() if len(p) == most)
    return dict(best[0][1]), best[0][0], best[1][0] if len(best) > 1 else np.inf


def test_the_scipy_assignment_equals_a_brute_force_up_to_six_by_six():
    rng = np.random.RandomState(11)
    checked = 0
    for trial in range(150):
        n, m = rng.randint(1, 7), rng.randint(1, 7)
        cost = rng.uniform(0.0, 0.8, (n, m))
        ok = rng.rand(n, m) < (0.35, 0.7, 1.0)[trial % 3]
        pairs, total = M.assign(cost, ok)
        want, want_total, second = brute(cost, ok)
        assert len(pairs) == len(want) and abs(total - want_total) < 1e-12, trial
        margin = M.margin_of(cost, ok, pairs, total)
        assert margin == np.inf if second == np.inf else abs(margin - (second - want_total)) < 1e-12, trial
        if second - want_total > 1e-9:
            assert pairs == want, trial
            checked += 1
    assert checked > 100


# ------------------------------------------------------------------------------------------------------------------ the GPU test's inputs

@pytest.fixture(scope="module")
def modelled():
    out = {}
    for name, (kw, recordings) in CS.scenarios().items():
        m = model(**kw)
        rows, iou, diag, frames = m.add_recordings([g for g, _d in recordings], [d for _g, d in recordings])
        out[name] = (m, rows, diag, [f for row in frames for f in row])
    kw, recordings = CS.untracked_case()                  # the end-to-end test's: the ids are the tracker's
    for name, recordings in (("tracked", CS.tracked_by_the_model(recordings)), ("perfect", CS.perfect_case()[1])):
        m = model(**kw)
        rows, iou, diag, frames = m.add_recordings([g for g, _d in recordings], [d for _g, d in recordings])
        out[name] = (m, rows, diag, [f for row in frames for f in row])
    return out


def test_every_frame_of_every_scenario_has_a_unique_optimum(modelled):
    """a condition on the inputs, not a tolerance: the device solver may differ from scipy only where the optimum is not unique"""
    total, least = 0, np.inf
    for name, (_m, _rows, diag, frames) in modelled.items():
        assert not diag[:, :4].any(), name                                                # no recording refused
        for f in frames:
            assert f["margin"] >= 1e-5, (name, f)
        total, least = total + len(frames), min([least] + [f["margin"] for f in frames])
    print(f"tracking evaluator scenarios: {total} frames, smallest uniqueness margin {least:.3g}")
    assert total >= 150 and max(f["n"] for f in modelled["crowd"][3]) == 65 and min(f["n"] for f in modelled["crowd"][3]) == 8


def test_the_scenarios_exercise_the_solver_the_carry_over_and_the_sizes(modelled):
    for name in ("crowd", "crowd_grid"):                                                  # iou_thre 0.2: a greedy kernel fails on these
        frames = modelled[name][3]
        differs = sum(f["greedy_differs"] for f in frames)
        print(f"{name}: the optimal matching differs from the greedy one in {differs} of {len(frames)} frames")
        assert 4 * differs >= len(frames)
    for name, (m, rows, diag, frames) in modelled.items():
        if name in ("tracked", "perfect"):                # their ids are not the generator's: the margin condition alone
            assert m.evaluate()["matches"] > 1000 and (m.evaluate()["idsw"] > 0) == (name == "tracked")
            continue
        assert any(f["carry_changes"] for f in frames), name
        e = m.evaluate()
        assert e["idsw"] > 0 and e["frag"] > 0 and e["fp"] > 0 and e["fn"] > 0 and e["mt"] > 0 and e["pt"] > 0, name
        assert diag[:, 4:].sum(axis=0).min() > 0, name                                    # every kind of dropped record occurs
    sizes = {(f["n"], f["m"]) for f in modelled["edge"][3]}
    assert sizes >= {(128, 128), (1, 0), (1, 1), (63, 64), (64, 63), (64, 65), (65, 64), (128, 63), (63, 128), (1, 128), (128, 1), (65, 65)}
    assert [int(r[2, 0]) for r in modelled["edge"][1]] == [24, 0, 1]                      # 24 frames (and a run of detections without labels), none, one
    assert int(modelled["edge"][1][0][2, M.C["gt_tracks"]]) == 128                        # what max_gt_tracks = 128 holds exactly


# ------------------------------------------------------------------------------------------------------------------ host checks

def test_the_limits_are_refused_on_the_host():
    from sast_amd.tracking import TrackingEvaluator
    TrackingEvaluator("gen1", False, iou_thre=1.0, max_gt_tracks=65536, max_labels_per_frame=128, max_hyp_per_frame=128)
    for kw in (dict(max_labels_per_frame=0), dict(max_labels_per_frame=129), dict(max_hyp_per_frame=0), dict(max_hyp_per_frame=129),
               dict(max_gt_tracks=0), dict(max_gt_tracks=65537), dict(iou_thre=0.0), dict(iou_thre=1.5), dict(iou_thre=float("nan")),
               dict(time_tol_us=-1)):
        with pytest.raises(ValueError, match="sast_amd.tracking"):
            TrackingEvaluator("gen4", True, **kw)
    te = TrackingEvaluator("gen4", True)
    assert te.classes == ("pedestrian", "two-wheeler", "car") and (te.min_box_diag, te.min_box_side) == (30, 10)
    e = te.evaluate()
    assert e["gt"] == 0 and math.isnan(e["MOTA"]) and set(te.per_class()) == set(te.classes) and not any(te.errors().values())


def test_the_argument_checks_and_no_cpu_fallback():
    from sast_amd.tracking import TrackingEvaluator
    te = TrackingEvaluator("gen1", False)
    gt, n = torch.zeros(2, 5, 10, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="gt must be a contiguous int32"):
        te.add_recordings(gt.float(), n, gt, n)
    with pytest.raises(ValueError, match="gt must be"):
        te.add_recordings(gt[:, :, :9].contiguous(), n, gt, n)
    with pytest.raises(ValueError, match="dt must be"):
        te.add_recordings(gt, n, torch.zeros(3, 5, 10, dtype=torch.int32), n)
    with pytest.raises(TypeError, match="n_dt must be"):
        te.add_recordings(gt, n, gt, n.int())
    with pytest.raises(ValueError, match="n_gt must be"):
        te.add_recordings(gt, torch.zeros(3, dtype=torch.int64), gt, n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.add_recordings(gt, n, gt, n)
    with pytest.raises(TypeError):
        te.merge(object())
    with pytest.raises(ValueError, match="same dataset"):
        te.merge(TrackingEvaluator("gen1", False, iou_thre=0.3))
    with pytest.raises(RuntimeError, match="rows follow"):
        te.rows
