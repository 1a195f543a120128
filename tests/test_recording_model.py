"""tests/recording_model.py (the numpy model of `PropheseeEvaluator.add_recordings`) against tests/golden/eval_recordings.npz, whose
windows are the reference's own filter_boxes + _match_times (tests/golden/make_golden_eval_recordings.py).  No GPU, no reference
(but for the one test that regenerates the file)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import make_golden_eval_recordings as G  # noqa: E402
import recording_model as RM  # noqa: E402

_FX = None


def fixture():
    global _FX
    if _FX is None:
        with np.load(os.path.join(GOLDEN, "eval_recordings.npz")) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def fixture_rows():
    fx = fixture()
    return [(RM.from_words(fx[f"gt{s}"]), RM.from_words(fx[f"dt{s}"])) for s in range(G.S)]


def _ref_available():
    import _ref_import as R
    return os.path.isdir(os.path.join(R.REF_ROOT, "utils", "evaluation", "prophesee"))


@pytest.mark.parametrize("tol", G.TOLS)
def test_model_reproduces_the_reference_windows_exactly(tol):
    fx, rows = fixture(), fixture_rows()
    want = {k: fx[f"tol{tol}/{k}"] for k in ("img_row", "img_t", "gt_ptr", "dt_ptr", "gt_idx", "dt_idx")}
    img_row, img_t, gt_ptr, dt_ptr, gt_idx, dt_idx = [], [], [0], [0], [], []
    for s, (gt, dt) in enumerate(rows):
        for t, gi, di, _n in RM.windows(gt, dt, tol, G.DIAG, G.SIDE):
            img_row.append(s), img_t.append(t)
            gt_idx += list(gi)
            dt_idx += list(di)
            gt_ptr.append(len(gt_idx)), dt_ptr.append(len(dt_idx))
    got = dict(img_row=img_row, img_t=img_t, gt_ptr=gt_ptr, dt_ptr=dt_ptr, gt_idx=gt_idx, dt_idx=dt_idx)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k], np.int64), v), k
    # and the flattened tables are those records, image ids in row order
    m = RM.Model(G.DIAG, G.SIDE)
    m.add_recordings(rows, tol=tol)
    tab = m.tables()
    assert np.array_equal(tab["image_t"], want["img_t"]) and not any(m.refused.values())
    assert np.array_equal(tab["gt_image_id"], np.repeat(np.arange(1, len(img_t) + 1), np.diff(want["gt_ptr"])))
    assert np.array_equal(tab["dt_image_id"], np.repeat(np.arange(1, len(img_t) + 1), np.diff(want["dt_ptr"])))
    for i in range(len(img_t)):
        gt, dt = rows[want["img_row"][i]]
        g, d = gt[want["gt_idx"][want["gt_ptr"][i]:want["gt_ptr"][i + 1]]], dt[want["dt_idx"][want["dt_ptr"][i]:want["dt_ptr"][i + 1]]]
        lo, hi = want["gt_ptr"][i], want["gt_ptr"][i + 1]
        assert np.array_equal(tab["gt_bbox"][lo:hi], np.stack([g[f] for f in "xywh"], 1)) and np.array_equal(tab["gt_category_id"][lo:hi], g["class_id"] + 1)
        lo, hi = want["dt_ptr"][i], want["dt_ptr"][i + 1]
        assert np.array_equal(tab["dt_bbox"][lo:hi], np.stack([d[f] for f in "xywh"], 1)) and np.array_equal(tab["dt_score"][lo:hi], d["class_confidence"])
        assert np.array_equal(tab["dt_category_id"][lo:hi], d["class_id"].astype(np.int64) + 1)


def test_fixture_inputs_regenerate_without_the_reference():
    for (g, d), (g2, d2) in zip(G.case_inputs(), fixture_rows()):
        assert RM.same_records(g, g2) and RM.same_records(d, d2)
        assert np.array_equal(g["track_id"], np.arange(len(g))) and np.array_equal(d["track_id"], np.arange(len(d)))


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_recordings_fixture():
    fx, new = fixture(), G.build()
    assert sorted(new) == sorted(fx)
    for k in fx:
        assert new[k].dtype == fx[k].dtype and np.array_equal(new[k], fx[k]), k


def test_fixture_covers_the_corner_cases():
    rows, fx = fixture_rows(), fixture()
    tol = 50000
    gt, dt = rows[0]
    gp, dp = RM.passes(gt, G.DIAG, G.SIDE), RM.passes(dt, G.DIAG, G.SIDE)
    img_t = fx[f"tol{tol}/img_t"][fx[f"tol{tol}/img_row"] == 0]
    assert len({len(g) for g, _d in rows}) == G.S and len({len(d) for _g, d in rows}) == G.S          # rows of different lengths
    assert (gt["t"] < 500000).any() and (gt["t"] == 500000).any() and (gt["t"] == 500001).any() and 500000 not in img_t
    size_ok = RM.passes(np.array([(600000,) + tuple(r)[1:] for r in gt], dtype=RM.BBOX_DTYPE), G.DIAG, G.SIDE)
    by_t = {int(t): size_ok[gt["t"] == t] for t in np.unique(gt["t"]) if t > 500000}
    assert any(not v.any() for v in by_t.values()) and any(v.any() and not v.all() for v in by_t.values())
    assert all((int(t) in img_t) == bool(v.any()) for t, v in by_t.items())
    assert np.any(np.diff(img_t) == 16000)
    member = [(dt["t"] >= t - tol) & (dt["t"] <= t + tol) for t in img_t]
    times = np.sum(member, 0)
    assert (times[dp] >= 3).any() and (times[dp] == 0).any()              # one detection in several images; detections in no window
    assert any(dp[m].sum() == 0 and m.sum() == 0 for m in member)         # an image with no detection
    for t in img_t:
        if all((dt["t"] == t + d).any() for d in (-tol - 1, -tol, tol, tol + 1)):
            break
    else:
        raise AssertionError("no image with detections at t +- tol and one microsecond further")
    assert any((m & (dt["t"] <= 500000)).any() for m in member)           # inside a window, before 0.5 s
    assert any((m & ~dp & (dt["t"] > 500000)).any() for m in member)      # inside a window, too small
    crowd = member[list(img_t).index(G.CROWD_T)] & dp & (dt["class_id"] == 0)
    assert crowd.sum() >= 130
    assert len(rows[1][0]) == 0 and len(rows[1][1]) > 0 and len(rows[2][0]) > 0 and len(rows[2][1]) == 0
    assert (gt["class_id"][gp] >= G.K).any() and (dt["class_id"][dp] >= G.K).any()
    m = RM.Model(G.DIAG, G.SIDE)
    m.add_recordings(rows, tol=tol)
    tab = m.tables()
    s, img = tab["dt_score"], tab["dt_image_id"]
    same = s[:, None] == s[None, :]
    assert (same & (img[:, None] == img[None, :]) & ~np.eye(len(s), dtype=bool)).any() and (same & (img[:, None] != img[None, :])).any()
    # a real measurement: AP strictly between 0 and 1, the precision table holds fractions
    stats, prec = CR.evaluate(*RM.coco_inputs(tab), G.K)
    print(stats)
    assert 0.0 < stats["AP"] < 1.0 and 0.0 < stats["AP_50"] < 1.0 and ((prec > 0) & (prec < 1)).any()


def test_model_counts_what_a_capacity_refuses():
    rows = fixture_rows()
    free = RM.Model(G.DIAG, G.SIDE)
    free.add_recordings(rows)
    n_img, n_dt = len(free.image_t), len(free.dt)
    for kw, key, n in ((dict(max_images=n_img - 2), "max_images", 2), (dict(max_labels=3), "max_labels_per_frame", None),
                       (dict(max_detections=n_dt - 1), "max_detections", None)):
        m = RM.Model(G.DIAG, G.SIDE, **kw)
        m.add_recordings(rows)
        assert m.refused[key] >= 1 and (n is None or m.refused[key] == n)
        assert sum(v for k, v in m.refused.items() if k != key) == 0
    m = RM.Model(G.DIAG, G.SIDE)
    m.add_recordings(rows, max_window=100)
    assert m.refused["max_window_detections"] == 1 and len(m.image_t) == n_img - 1
    bad = rows[0][1].copy()
    bad["t"][5] = bad["t"][4] - 1
    m = RM.Model(G.DIAG, G.SIDE)
    m.add_recordings([(rows[0][0], bad), rows[2]])
    assert m.refused["unsorted"] == 1 and len(m.image_t) == len(np.unique(rows[2][0]["t"][RM.passes(rows[2][0], G.DIAG, G.SIDE)]))
