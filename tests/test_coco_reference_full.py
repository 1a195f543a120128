"""tests/coco_reference_full.py (COCOeval's precision, recall and score tables at maxDets 1 / 10 / 100 and the twelve stats, the
yardstick of tests/test_evaluation_summary.py) pinned on the CPU: its maxDets-100 precision slice is tests/coco_reference.py's table
bit for bit on the committed fixture, and cases whose numbers can be derived by hand.  "1.0" below is tp / (tp + 0 + eps) as COCOeval
computes it: 1 / (1 + 2^-52) for tp = 1.  Parity with pycocotools itself stays unpinned: it is not installed where this project is
built."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import coco_reference_full as CF  # noqa: E402
import make_golden_eval as G  # noqa: E402

EPS = np.spacing(1)
ONE = 1.0 / (1.0 + EPS)


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
    d["score"] = r[:, 6].astype(np.float32).astype(np.float64)
    return d


def _f32(v):
    return float(np.float32(v))


def test_keys_and_shapes():
    assert CF.MAX_DETS == (1, 10, 100) and CF.STAT_KEYS[:6] == CR.OUT_KEYS and len(CF.STAT_KEYS) == 12
    t = CF.accumulate(1, _gt([(1, 1, 10, 10, 40, 40)]), _dt([(1, 1, 10, 10, 40, 40, 0.5)]), 2)
    assert t["precision"].shape == t["scores"].shape == (10, 101, 2, 4, 3) and t["recall"].shape == (10, 2, 4, 3)


def test_the_maxdets_100_slice_is_the_precision_table_bit_for_bit_on_the_fixture():
    with np.load(os.path.join(GOLDEN, "prophesee_eval.npz")) as z:
        fx = {k: z[k] for k in z.files}
    for name in sorted(G.CASES):
        t = {k: fx[f"{name}/{k}"] for k in G.TABLE_KEYS}
        gt = {"image_id": t["gt_image_id"], "category_id": t["gt_category_id"], "bbox": t["gt_bbox"], "area": t["gt_area"]}
        dt = {"image_id": t["dt_image_id"], "category_id": t["dt_category_id"], "bbox": t["dt_bbox"], "area": t["dt_area"], "score": t["dt_score"]}
        K = G.N_CLASSES[G.CASES[name][0]]
        stats, full = CF.evaluate(int(t["n_images"]), gt, dt, K)
        six, prec = CR.evaluate(int(t["n_images"]), gt, dt, K)
        assert np.array_equal(full["precision"][..., 2].view(np.int64), prec.view(np.int64)), name
        assert all(stats[k] == six[k] for k in CR.OUT_KEYS)
        # the fixture separates the three maxDets: recall grows strictly, and the precision tables differ
        print(name, {k: round(stats[k], 4) for k in ("AR_1", "AR_10", "AR_100")},
              "precision entries that differ 1|10, 10|100:", [int((full["precision"][..., i] != full["precision"][..., i + 1]).sum()) for i in (0, 1)])
        assert 0.0 < stats["AR_1"] < stats["AR_10"] < stats["AR_100"] < 1.0, (name, stats)
        assert all((full["precision"][..., i] != full["precision"][..., i + 1]).sum() > 1000 for i in (0, 1))
        # -1 and 0 sit where the precision has them; elsewhere a score is one of the detections' scores
        p, s = full["precision"], full["scores"]
        assert np.array_equal(s == -1, p == -1) and np.all(np.isin(s[p > 0], t["dt_score"])) and np.all(s[:, 1:][p[:, 1:] == 0] == 0)
        assert np.array_equal(full["recall"] == -1, (p == -1).all(axis=1))


def test_tp_fp_tp_by_hand():
    g = [(1, 1, 10, 10, 40, 40), (1, 1, 100, 100, 40, 40)]
    d = [(1, 1, 10, 10, 40, 40, 0.9), (1, 1, 200, 10, 40, 40, 0.8), (1, 1, 100, 100, 40, 40, 0.7)]
    stats, t = CF.evaluate(1, _gt(g), _dt(d), 1)
    p, r, s = t["precision"], t["recall"], t["scores"]
    for a in (0, 2):                                   # 40 x 40 = 1600: all areas and medium
        assert np.all(r[:, 0, a, 0] == 0.5) and np.all(r[:, 0, a, 1] == 1.0) and np.all(r[:, 0, a, 2] == 1.0)
        # m = 1: only the 0.9 detection is kept: recall 0.5 at precision 1
        assert np.all(p[:, :51, 0, a, 0] == ONE) and np.all(p[:, 51:, 0, a, 0] == 0.0)
        assert np.all(s[:, :51, 0, a, 0] == _f32(0.9)) and np.all(s[:, 51:, 0, a, 0] == 0.0)
        for m in (1, 2):                               # tp, fp, tp: the envelope is 1 up to recall 0.5, 2/3 beyond
            assert np.all(p[:, :51, 0, a, m] == ONE) and np.all(p[:, 51:, 0, a, m] == 2.0 / (3.0 + EPS))
            assert np.all(s[:, :51, 0, a, m] == _f32(0.9)) and np.all(s[:, 51:, 0, a, m] == _f32(0.7))
    for a in (1, 3):                                   # no small and no large label
        assert np.all(p[:, :, 0, a, :] == -1) and np.all(r[:, 0, a, :] == -1) and np.all(s[:, :, 0, a, :] == -1)
    assert (stats["AR_1"], stats["AR_10"], stats["AR_100"], stats["AR_M"]) == (0.5, 1.0, 1.0, 1.0)
    assert stats["AR_S"] == -1.0 and stats["AR_L"] == -1.0 and stats["AP_S"] == -1.0
    assert abs(stats["AP"] - (51 + 50 * 2 / 3) / 101) < 1e-15
    pc = CF.per_class(t, ("thing",))
    assert pc == {"thing": {"AP": stats["AP"], "AP_50": stats["AP_50"], "AP_75": stats["AP_75"], "AR_100": 1.0}}


def test_no_detections_recall_zero_where_there_are_labels_and_twelve_zeros():
    g = _gt([(1, 1, 10, 10, 40, 40)])
    t = CF.accumulate(1, g, _dt([]), 2)
    for a in (0, 2):
        assert np.all(t["recall"][:, 0, a, :] == 0.0) and np.all(t["precision"][:, :, 0, a, :] == 0.0) and np.all(t["scores"][:, :, 0, a, :] == 0.0)
    assert np.all(t["recall"][:, 0, [1, 3], :] == -1) and np.all(t["recall"][:, 1] == -1) and np.all(t["precision"][:, :, 1] == -1)
    stats, none = CF.evaluate(1, g, _dt([]), 2)
    assert none is None and stats == {k: 0.0 for k in CF.STAT_KEYS} and list(stats) == list(CF.STAT_KEYS)


def test_a_category_without_labels_is_minus_one():
    g = [(1, 1, 10, 10, 40, 40)]
    d = [(1, 1, 10, 10, 40, 40, 0.9), (1, 2, 10, 10, 40, 40, 0.8)]
    stats, t = CF.evaluate(1, _gt(g), _dt(d), 2)
    assert np.all(t["precision"][:, :, 1] == -1) and np.all(t["recall"][:, 1] == -1) and np.all(t["scores"][:, :, 1] == -1)
    assert np.all(t["recall"][:, 0, 0, :] == 1.0) and stats["AR_1"] == 1.0          # the mean skips the -1 category
    pc = CF.per_class(t, ("a", "b"))
    assert pc["b"] == {"AP": -1.0, "AP_50": -1.0, "AP_75": -1.0, "AR_100": -1.0} and pc["a"]["AR_100"] == 1.0


def test_the_eleventh_detection_is_the_only_match():
    g = [(1, 1, 10, 10, 40, 40)]
    d = [(1, 1, 300 + 50 * i, 300, 40, 40, 0.9 - 0.01 * i) for i in range(10)] + [(1, 1, 10, 10, 40, 40, 0.5)]
    stats, t = CF.evaluate(1, _gt(g), _dt(d), 1)
    r, p, s = t["recall"], t["precision"], t["scores"]
    assert np.all(r[:, 0, 0, 0] == 0.0) and np.all(r[:, 0, 0, 1] == 0.0) and np.all(r[:, 0, 0, 2] == 1.0)
    assert (stats["AR_1"], stats["AR_10"], stats["AR_100"]) == (0.0, 0.0, 1.0)
    # m = 1, 10: false positives only -- threshold 0 is reached at the first of them (precision 0, its score), nothing beyond
    for m in (0, 1):
        assert np.all(p[:, :, 0, 0, m] == 0.0) and np.all(s[:, 0, 0, 0, m] == _f32(0.9)) and np.all(s[:, 1:, 0, 0, m] == 0.0)
    # m = 100: the match is the 11th: precision 1 / 11 everywhere; threshold 0 carries the first detection's score, the others the 11th's
    assert np.all(p[:, :, 0, 0, 2] == 1.0 / (11.0 + EPS))
    assert np.all(s[:, 0, 0, 0, 2] == _f32(0.9)) and np.all(s[:, 1:, 0, 0, 2] == _f32(0.5))


def test_an_ignored_top_record_still_gives_its_score_to_threshold_zero():
    # medium range: the top-scored detection is large and unmatched there -> ignored; the second matches the medium label
    g = [(1, 1, 10, 10, 40, 40), (1, 1, 200, 200, 120, 120)]
    d = [(1, 1, 200, 200, 120, 120, 0.9), (1, 1, 10, 10, 40, 40, 0.6)]
    _stats, t = CF.evaluate(1, _gt(g), _dt(d), 1)
    p, s, r = t["precision"], t["scores"], t["recall"]
    for m in (1, 2):
        assert np.all(r[:, 0, 2, m] == 1.0) and np.all(p[:, :, 0, 2, m] == ONE)
        assert np.all(s[:, 0, 0, 2, m] == _f32(0.9)) and np.all(s[:, 1:, 0, 2, m] == _f32(0.6))
    # at maxDets 1 the one kept record is the ignored one: no recall, and still its score at threshold 0
    assert np.all(r[:, 0, 2, 0] == 0.0) and np.all(p[:, :, 0, 2, 0] == 0.0)
    assert np.all(s[:, 0, 0, 2, 0] == _f32(0.9)) and np.all(s[:, 1:, 0, 2, 0] == 0.0)
    # over all areas nothing is ignored
    assert np.all(r[:, 0, 0, 0] == 0.5) and np.all(r[:, 0, 0, 2] == 1.0) and np.all(s[:, 51:, 0, 0, 2] == _f32(0.6))
