"""Fixture of `PropheseeEvaluator.add_recordings`: `python tests/golden/make_golden_eval_recordings.py` -> eval_recordings.npz.

Three recordings as sorted Prophesee box records (labels and detections), built from seeded numpy draws to contain the corner cases
tests/test_recording_model.py::test_fixture_covers_the_corner_cases asserts, and next to them what the REFERENCE'S OWN code makes of
them: filter_boxes (utils/evaluation/prophesee/io/box_filtering.py) with gen1's thresholds on labels and detections, np.unique of the
label timestamps and _match_times (metrics/coco_eval.py:46-90), per recording, for time_tol 0, 1000 and 50000.  Every record carries its
index in its row as `track_id` (a field no evaluation reads), so the reference's windows are stored as INDICES into the inputs: data
only.  coco_eval.py imports pycocotools at module scope; it is not installed, so two empty stub modules stand in (COCOeval is never
run here).  The reference is needed for `build()` alone: `case_inputs()` and the tests of the committed file run without it."""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recording_model as RM  # noqa: E402

OUT = os.path.join(HERE, "eval_recordings.npz")
DIAG, SIDE, K = 30, 10, 2          # gen1
TOLS = (0, 1000, 50000)
S = 3
W, H = 304, 240
CROWD_T = 1400000                  # the image with more than 100 detections of one category in its window


def _q(v):
    """quarter pixels: coordinates, sizes and their sums are exact in fp32"""
    return np.round(np.asarray(v, dtype=np.float64) * 4) / 4


def case_inputs():
    """-> [(gt records, dt records)] * S, sorted by t, track_id = the record's index in its row"""
    rs = np.random.RandomState(2024)

    def label_box():
        w, h = _q(rs.uniform(12, 120)), _q(rs.uniform(12, 100))
        return (_q(rs.uniform(0, W - 1 - w)), _q(rs.uniform(0, H - 1 - h)), w, h, int(rs.randint(K)))

    def det_of(boxes):
        if boxes and rs.rand() < 0.7:      # a jittered copy of a label, mostly of its class
            x, y, w, h, c = boxes[rs.randint(len(boxes))]
            j = rs.uniform(-0.2, 0.2, 4)
            x, y, w, h = _q(x + j[0] * w), _q(y + j[1] * h), _q(w * (1 + j[2])), _q(h * (1 + j[3]))
            c = c if rs.rand() < 0.8 else int(rs.randint(K))
        else:
            x, y, w, h, c = label_box()
        if rs.rand() < 0.15:               # too small for the filter
            w = _q(rs.uniform(1, 9))
        return (x, y, max(w, 0.25), max(h, 0.25), c, rs.randint(1, 33) / 32.0)      # 32 score levels: ties within and across images

    rows = []
    # ---- recording 0: every corner case
    gt, dt = [], []
    labels_at = {}

    def put(t, boxes):
        labels_at[t] = boxes
        gt.extend((t,) + b for b in boxes)

    def dets(t, n, boxes):
        dt.extend((t,) + det_of(boxes) for _ in range(n))

    put(400000, [label_box(), label_box()])                         # before 0.5 s
    put(500000, [label_box()])                                      # exactly 0.5 s: the filter wants t > 500000
    put(500001, [label_box(), label_box()])                         # the first image; its window reaches back before 0.5 s
    dets(460000, 3, labels_at[500001])                              # inside the window, but t <= 500000: out
    dets(500000, 2, labels_at[500001])
    dets(500001, 4, labels_at[500001])
    dets(540000, 3, labels_at[500001])
    put(600000, [(10, 10, 9.75, 150, 0), (50, 20, 15, 15, 1)])       # every label fails the size filter: no image
    dets(600000, 5, [(10, 10, 60, 60, 0)])                          # ... so these (and those at 640000) are in no window
    dets(640000, 2, [])
    put(700000, [label_box(), (30, 30, 9.75, 40, 0), label_box(), (60, 60, 18, 23.75, 1), (5, 5, 40, 40, 5)])   # partly failing; a class id >= K
    dets(700000, 6, labels_at[700000][:1] + labels_at[700000][2:3])
    dt.append((700000, 5, 5, 40, 40, 7, 0.75))                      # a detection of a class id >= K
    for t in (800000, 816000, 832000):                              # 16 ms apart with tol 50 ms: one detection in several images
        put(t, [label_box() for _ in range(3)])
    for t in (760000, 790000, 810000, 824000, 850000, 881000, 882000, 882001):
        dets(t, 3, labels_at[816000])
    put(1000000, [label_box(), label_box()])
    for t in (949999, 950000, 1000000, 1050000, 1050001):           # exactly t +- tol (in) and one microsecond further (out)
        dets(t, 2, labels_at[1000000])
    put(1200000, [label_box()])                                     # an image with no detection
    dets(1300000, 4, [])                                            # detections in no window
    put(CROWD_T, [label_box()[:4] + (0,) for _ in range(5)])
    crowd = [det_of(labels_at[CROWD_T]) for _ in range(170)]
    big = [d[:2] + (max(d[2], 24.0), max(d[3], 24.0), 0, d[5]) for d in crowd[:130]]         # 130 of category 0 pass the filter
    for i, d in enumerate(big + crowd[130:]):
        dt.append((CROWD_T - 40000 + 500 * i,) + d)
    rows.append((gt, dt))
    # ---- recording 1: detections, no label
    rows.append(([], [(t,) + det_of([]) for t in (550000, 700000, 700000, 900000, 1100000)]))
    # ---- recording 2: labels, no detection
    gt = []
    for t in (480000, 620000, 620000 + 16667, 900000):
        gt.extend((t,) + label_box() for _ in range(1 + rs.randint(4)))
    rows.append((gt, []))

    out = []
    for gt, dt in rows:
        g, d = RM.records(len(gt)), RM.records(len(dt))
        for i, (t, x, y, w, h, c) in enumerate(gt):
            g[i] = (t, x, y, w, h, c, i, 1.0)
        for i, (t, x, y, w, h, c, s) in enumerate(sorted(dt, key=lambda r: r[0])):      # stable: equal t keep their order
            d[i] = (t, x, y, w, h, c, i, s)
        assert RM.is_sorted(g) and RM.is_sorted(d)
        out.append((g, d))
    return out


def _reference():
    sys.path.insert(0, HERE)
    import _ref_import as R
    if not os.path.isdir(os.path.join(R.REF_ROOT, "utils", "evaluation", "prophesee")):
        raise RuntimeError(f"reference not found under {R.REF_ROOT}")
    sys.dont_write_bytecode = True
    if "pycocotools" not in sys.modules:               # coco_eval.py:14-21 imports it at module scope; COCOeval is never run here
        m, mc, me = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.coco"), types.ModuleType("pycocotools.cocoeval")
        mc.COCO = type("COCO", (), {})
        me.COCOeval = type("COCOeval", (), {})
        m.coco, m.cocoeval = mc, me
        sys.modules.update({"pycocotools": m, "pycocotools.coco": mc, "pycocotools.cocoeval": me})
    if R.REF_ROOT not in sys.path:
        sys.path.insert(0, R.REF_ROOT)
    from utils.evaluation.prophesee.io.box_filtering import filter_boxes
    from utils.evaluation.prophesee.metrics import coco_eval
    return filter_boxes, coco_eval._match_times


def reference_windows(rows, tol):
    """-> img_row, img_t int64 [I]; gt_ptr, dt_ptr int64 [I + 1]; gt_idx, dt_idx int64: image i holds the labels gt_idx[gt_ptr[i] :
    gt_ptr[i + 1]] and the detections dt_idx[dt_ptr[i] : dt_ptr[i + 1]] of its row, as indices into the unfiltered inputs"""
    filter_boxes, match_times = _reference()
    img_row, img_t, gt_ptr, dt_ptr, gt_idx, dt_idx = [], [], [0], [0], [], []
    for s, (gt, dt) in enumerate(rows):
        gt_f, dt_f = filter_boxes(gt, int(5e5), DIAG, SIDE), filter_boxes(dt, int(5e5), DIAG, SIDE)   # evaluation.py:33-38
        assert np.all(gt_f['t'][1:] >= gt_f['t'][:-1]) and np.all(dt_f['t'][1:] >= dt_f['t'][:-1])     # coco_eval.py:43-44
        all_ts = np.unique(gt_f['t'])
        gt_win, dt_win = match_times(all_ts, gt_f, dt_f, tol)
        for t, g, d in zip(all_ts, gt_win, dt_win):
            img_row.append(s), img_t.append(int(t))
            gt_idx += [int(i) for i in g['track_id']]
            dt_idx += [int(i) for i in d['track_id']]
            gt_ptr.append(len(gt_idx)), dt_ptr.append(len(dt_idx))
    return {k: np.asarray(v, dtype=np.int64) for k, v in (("img_row", img_row), ("img_t", img_t), ("gt_ptr", gt_ptr), ("dt_ptr", dt_ptr),
                                                           ("gt_idx", gt_idx), ("dt_idx", dt_idx))}


def build() -> dict:
    rows = case_inputs()
    out = {}
    for s, (gt, dt) in enumerate(rows):
        out[f"gt{s}"], out[f"dt{s}"] = RM.words(gt), RM.words(dt)
    for tol in TOLS:
        for k, v in reference_windows(rows, tol).items():
            out[f"tol{tol}/{k}"] = v
    return out


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {t: len(arrays[f"tol{t}/img_t"]) for t in TOLS}, "images,",
          {t: len(arrays[f"tol{t}/dt_idx"]) for t in TOLS}, "detection memberships")
