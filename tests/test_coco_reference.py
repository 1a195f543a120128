"""tests/coco_reference.py (the numpy fp64 restatement of COCOeval that tests/test_evaluation.py measures the device evaluator against)
pinned by cases whose numbers can be derived by hand.  pycocotools is not a dependency of this project, so the restatement's parity
with pycocotools itself is not pinned by any test; these cases and a reading of cocoeval.py are what stands behind it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_reference as CR  # noqa: E402


def _gt(rows):
    """rows: (image_id, category_id, x, y, w, h)"""
    r = np.asarray(rows, np.float64).reshape(-1, 6)
    b = r[:, 2:6].astype(np.float32)
    return {"image_id": r[:, 0].astype(np.int64), "category_id": r[:, 1].astype(np.int64), "bbox": b,
            "area": (b[:, 2] * b[:, 3]).astype(np.float64)}


def _dt(rows):
    """rows: (image_id, category_id, x, y, w, h, score)"""
    r = np.asarray(rows, np.float64).reshape(-1, 7)
    d = _gt(r[:, :6])
    d["score"] = r[:, 6].astype(np.float32)
    return d


def test_thresholds_are_pycocotools_params():
    assert CR.IOU_THRS.shape == (10,) and CR.IOU_THRS[0] == 0.5 and CR.IOU_THRS[5] == 0.75
    assert CR.REC_THRS.shape == (101,) and CR.REC_THRS[0] == 0.0 and CR.REC_THRS[50] == 0.5 and CR.REC_THRS[100] == 1.0
    assert CR.AREA_RNG == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_iou_is_one_rounding_per_operation():
    assert CR.iou_xywh([0, 0, 48, 64], [0, 0, 48, 128]) == 0.5
    assert CR.iou_xywh([0, 0, 10, 10], [10, 0, 10, 10]) == 0.0          # touching: iw == 0
    assert CR.iou_xywh([0, 0, 10, 10], [5, 5, 10, 10]) == 25.0 / 175.0


def test_detections_equal_to_the_labels_give_one_for_present_sizes_and_minus_one_for_absent():
    # a small (20 x 20) and a large (100 x 100) box; no medium one
    g = [(1, 1, 10, 10, 20, 20), (1, 1, 100, 50, 100, 100), (2, 1, 30, 30, 20, 20)]
    stats, prec = CR.evaluate(2, _gt(g), _dt([r + (0.9,) for r in g]), 1)
    # "1.0" is tp / (tp + 0 + eps): exactly 1 from tp = 2 on, 1 / (1 + 2^-52) = 1 - 2^-52 for the single large box
    assert stats["AP_M"] == -1.0 and stats["AP_S"] == 1.0 and stats["AP_L"] == 1.0 / (1.0 + np.spacing(1))
    for k in ("AP", "AP_50", "AP_75"):
        assert abs(stats[k] - 1.0) <= 2.0 ** -52
    assert prec.shape == (10, 101, 1, 4) and np.all(prec[:, :, 0, 2] == -1) and np.all(prec[:, :, 0, [0, 1]] == 1.0)
    assert np.all(prec[:, :, 0, 3] == 1.0 - 2.0 ** -52)


def test_tp_fp_tp_gives_the_hand_computed_ap50():
    g = [(1, 1, 10, 10, 40, 40), (1, 1, 100, 100, 40, 40)]
    d = [(1, 1, 10, 10, 40, 40, 0.9), (1, 1, 200, 10, 40, 40, 0.8), (1, 1, 100, 100, 40, 40, 0.7)]
    stats, prec = CR.evaluate(1, _gt(g), _dt(d), 1)
    # recall 0.5 at precision 1, then (0.5, 0.5), then (1, 2/3): the envelope is 1 up to recall 0.5 (51 thresholds), 2/3 beyond (50)
    want = (51 * 1.0 + 50 * (2.0 / (1.0 + 2.0 + np.spacing(1)))) / 101
    assert abs(stats["AP_50"] - (51 * 1 + 50 * (2 / 3)) / 101) < 1e-15 and abs(stats["AP_50"] - want) < 1e-15
    assert np.all(prec[:, :51, 0, 0] == 1.0 / (1.0 + np.spacing(1))) and np.all(prec[0, 51:, 0, 0] == 2.0 / (3.0 + np.spacing(1)))
    for k in ("AP", "AP_75", "AP_M"):   # the detections are exact copies: every threshold gives the same row
        assert abs(stats[k] - stats["AP_50"]) < 1e-12
    assert stats["AP_S"] == -1.0 and stats["AP_L"] == -1.0


def test_a_category_with_labels_and_no_detections_gives_zero():
    g = [(1, 1, 10, 10, 40, 40), (1, 2, 100, 100, 40, 40)]
    stats, prec = CR.evaluate(1, _gt(g), _dt([(1, 1, 10, 10, 40, 40, 0.9)]), 2)
    assert np.all(prec[:, :, 0, 0] == 1.0 - 2.0 ** -52) and np.all(prec[:, :, 1, 0] == 0.0)
    assert abs(stats["AP"] - 0.5) <= 2.0 ** -52 and abs(stats["AP_M"] - 0.5) <= 2.0 ** -52 and stats["AP_S"] == -1.0


def test_no_detections_at_all_gives_six_zeros():
    stats, prec = CR.evaluate(1, _gt([(1, 1, 10, 10, 40, 40)]), _dt([]), 2)
    assert prec is None and stats == {k: 0.0 for k in CR.OUT_KEYS}


def test_matching_rules_ties_ignore_flags_and_the_cut_to_100():
    # equal IoU: the later ground truth replaces the earlier one (`iou < best` skips, equality does not)
    g = [(1, 1, 0, 0, 40, 40), (1, 1, 0, 0, 40, 40)]
    e = CR.evaluate_img([{"bbox": r[2:], "area": 1600.0} for r in g], [{"bbox": (0, 0, 40, 40), "area": 1600.0, "score": 0.5}], CR.AREA_RNG[0])
    assert e[1].all() and e[3] == 2
    # a detection whose only overlap is an out-of-range ground truth is matched to it and ignored, not a false positive
    e = CR.evaluate_img([{"bbox": (0, 0, 40, 40), "area": 1600.0}], [{"bbox": (0, 0, 40, 40), "area": 1600.0, "score": 0.5}], CR.AREA_RNG[1])
    assert e[1].all() and e[2].all() and e[3] == 0
    # unmatched and out of range: ignored; unmatched in range: a false positive
    e = CR.evaluate_img([], [{"bbox": (0, 0, 40, 40), "area": 1600.0, "score": 0.5}], CR.AREA_RNG[1])
    assert not e[1].any() and e[2].all()
    e = CR.evaluate_img([], [{"bbox": (0, 0, 40, 40), "area": 1600.0, "score": 0.5}], CR.AREA_RNG[2])
    assert not e[1].any() and not e[2].any()
    # 130 detections: the 100 best by a stable sort on the score
    d = [{"bbox": (0, 0, 40, 40), "area": 1600.0, "score": (i % 13) / 13.0, "i": i} for i in range(130)]
    e = CR.evaluate_img([], d, CR.AREA_RNG[0])
    want = sorted(range(130), key=lambda i: (-d[i]["score"], i))[:100]
    assert e[0] == [d[i]["score"] for i in want] and e[1].shape == (10, 100)
    assert CR.evaluate_img([], [], CR.AREA_RNG[0]) is None
