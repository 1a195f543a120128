"""Fixtures of the Prophesee mAP evaluator (sast_amd/evaluation.py): `python tests/golden/make_golden_eval.py` -> prophesee_eval.npz.

Every expected table comes from the reference's own code, imported from the reference root that `_ref_import.py` names: to_prophesee
(utils/evaluation/prophesee/io/box_loading.py) on ObjectLabels and post-processed prediction tensors, filter_boxes
(io/box_filtering.py) with the thresholds of evaluate_list (evaluation.py:22-38), then evaluate_detection's loop over "files"
(metrics/coco_eval.py:40-52: np.unique of the timestamps, _match_times) with one frame per file, and _to_coco_format.  The reference's
coco_eval.py imports pycocotools at module scope; it is not installed, so a stub stands in and COCOeval itself is never run here.  The
one thing added to the reference's tables is the detections' area, which COCO.loadRes would compute as bbox[2] * bbox[3] on the fp32
fields: it is restated here in one line (`dt_area`).

Inputs (seeded numpy draws, rounded to quarter pixels so that sums and the threshold cases are exact) are stored next to the tables:
three cases -- gen1, gen4, gen4 with downsample_by_2 -- whose frames are built to contain the corner cases that
tests/test_evaluation.py::test_fixture_covers_the_corner_cases asserts.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "prophesee_eval.npz")

M_ROWS = 12      # label rows per frame
A_ROWS = 160     # detection rows per frame
N_FRAMES = 18
CASES = {
    # name: (dataset, downsample_by_2, (height, width), seed)
    "gen1": ("gen1", False, (240, 304), 11),
    "gen4": ("gen4", False, (720, 1280), 12),
    "gen4_ds2": ("gen4", True, (360, 640), 13),
}
N_CLASSES = {"gen1": 2, "gen4": 3}
TABLE_KEYS = ("n_images", "gt_image_id", "gt_category_id", "gt_bbox", "gt_area", "gt_id", "dt_image_id", "dt_category_id", "dt_score",
              "dt_bbox", "dt_area")


def thresholds(dataset: str, downsample_by_2: bool):
    diag, side = (60, 20) if dataset == "gen4" else (30, 10)
    return (diag // 2, side // 2) if downsample_by_2 else (diag, side)


def _q(v):
    """quarter pixels: every coordinate, size and sum of two of them is exact in fp32"""
    return np.round(np.asarray(v, dtype=np.float64) * 4) / 4


def case_inputs(name: str):
    """-> labels fp32 [N, M, 7], counts int32 [N], det fp32 [N, A, 7], n_det int32 [N] (rows past the counts are zero)"""
    dataset, ds2, (H, W), seed = CASES[name]
    K = N_CLASSES[dataset]
    diag, side = thresholds(dataset, ds2)
    u = diag / 30.0                                   # the unit the hand-made boxes scale with: 1 (gen1, gen4 halved) or 2 (gen4)
    rs = np.random.RandomState(seed)
    labels = np.zeros((N_FRAMES, M_ROWS, 7), np.float32)
    counts = np.zeros(N_FRAMES, np.int32)
    det = np.zeros((N_FRAMES, A_ROWS, 7), np.float32)
    n_det = np.zeros(N_FRAMES, np.int32)

    def put_labels(n, t, rows):
        counts[n] = len(rows)
        for i, (x, y, w, h, c) in enumerate(rows):
            labels[n, i] = (t, x, y, w, h, c, 1.0)

    def put_dets(n, rows):
        n_det[n] = len(rows)
        for i, (x, y, w, h, s, c) in enumerate(rows):
            det[n, i] = (x, y, x + w, y + h, 0.5, s, c)

    def random_labels(k, classes):
        rows = []
        for _ in range(k):
            w, h = _q(rs.uniform(0.2, 5.0) * diag), _q(rs.uniform(0.2, 5.0) * diag)
            w, h = min(w, W / 2), min(h, H / 2)
            rows.append((_q(rs.uniform(0, W - 1 - w)), _q(rs.uniform(0, H - 1 - h)), w, h, classes[rs.randint(len(classes))]))
        return rows

    def random_dets(k, gts, classes):
        rows = []
        for _ in range(k):
            if gts and rs.rand() < 0.6:                # a jittered copy of a label, often of its class
                x, y, w, h, c = gts[rs.randint(len(gts))]
                j = rs.uniform(-0.25, 0.25, 4)
                x, y, w, h = _q(x + j[0] * w), _q(y + j[1] * h), _q(w * (1 + j[2])), _q(h * (1 + j[3]))
                c = c if rs.rand() < 0.8 else rs.randint(K)
            else:
                x, y, w, h, c = random_labels(1, list(range(K)))[0]
            rows.append((x, y, max(w, 0.25), max(h, 0.25), rs.randint(1, 65) / 64.0, c))   # 64 score levels: ties within and across frames
        return rows

    all_classes = list(range(K))
    seen = [0, 2] if K == 3 else [0, 1]               # gen4: no label is ever a two-wheeler, detections are
    t = 600000
    for n in range(N_FRAMES):
        t += 50000
        if n == 0:      # before 0.5 s: neither labels nor detections count
            rows = random_labels(3, seen)
            put_labels(n, 400000, rows)
            put_dets(n, random_dets(20, rows, all_classes))
        elif n == 1:    # exactly 0.5 s: the filter wants t > 500000
            rows = random_labels(2, seen)
            put_labels(n, 500000, rows)
            put_dets(n, random_dets(10, rows, all_classes))
        elif n == 2:    # every label falls to the size filter, the detections would pass it
            put_labels(n, t, [(10, 10, side - 0.25, 5 * diag, 0), (50, 20, 0.5 * diag, 0.5 * diag, seen[1])])
            put_dets(n, random_dets(12, [(10, 10, 2 * diag, 2 * diag, 0)], all_classes))
        elif n == 3:    # not a frame (counts == 0), with detections
            put_dets(n, random_dets(8, [], all_classes))
        elif n == 4:    # boxes exactly on and a quarter pixel under the diagonal and side thresholds; IoU exactly 0.5
            rows = [(8, 8, 18 * u, 24 * u, 0), (40 * u, 8, 18 * u - 0.25, 24 * u, 0), (80 * u, 8, side, 3 * diag, seen[1]),
                    (100 * u, 8, side - 0.25, 3 * diag, seen[1]), (8, 110 * u, 24 * u, 64 * u, 0)]
            put_labels(n, t, rows)
            put_dets(n, [(8, 8, 18 * u, 24 * u, 0.75, 0), (40 * u, 8, 24 * u, 18 * u - 0.25, 0.75, 0), (80 * u, 8, 3 * diag, side, 0.5, seen[1]),
                         (8, 110 * u, 24 * u, 32 * u, 0.5, 0)] + random_dets(6, rows, all_classes))
        elif n == 5:    # more than 100 detections of one category survive the filter
            rows = random_labels(6, [0])
            put_labels(n, t, rows)
            dets = [r[:5] + (0,) for r in random_dets(150, rows, [0])]
            put_dets(n, dets)
        elif n == 6:    # a timestamp fp32 cannot hold exactly
            rows = random_labels(4, seen)
            put_labels(n, 3123456789.0, rows)
            put_dets(n, random_dets(30, rows, all_classes))
        elif n == 7:    # labels, no detection
            put_labels(n, t, random_labels(5, seen))
        else:
            rows = random_labels(rs.randint(1, M_ROWS + 1), seen)
            put_labels(n, t, rows)
            put_dets(n, random_dets(rs.randint(0, 90), rows, all_classes))
    return labels, counts, det, n_det


def _reference():
    sys.path.insert(0, HERE)
    import _ref_import as R
    if not os.path.isdir(os.path.join(R.REF_ROOT, "utils", "evaluation", "prophesee")):
        raise RuntimeError(f"reference not found under {R.REF_ROOT}")
    sys.dont_write_bytecode = True
    R._install_stubs()
    if "pycocotools" not in sys.modules:               # coco_eval.py:14-21 imports it at module scope; COCOeval is never run here
        m, mc, me = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.coco"), types.ModuleType("pycocotools.cocoeval")
        mc.COCO = type("COCO", (), {})
        me.COCOeval = type("COCOeval", (), {})
        m.coco, m.cocoeval = mc, me
        sys.modules.update({"pycocotools": m, "pycocotools.coco": mc, "pycocotools.cocoeval": me})
    if R.REF_ROOT not in sys.path:
        sys.path.insert(0, R.REF_ROOT)
    from data.genx_utils.labels import ObjectLabels
    from utils.evaluation.prophesee.io.box_filtering import filter_boxes
    from utils.evaluation.prophesee.io.box_loading import to_prophesee
    from utils.evaluation.prophesee.metrics import coco_eval
    return ObjectLabels, to_prophesee, filter_boxes, coco_eval


def reference_tables(name: str, labels, counts, det, n_det):
    import torch
    ObjectLabels, to_prophesee, filter_boxes, coco_eval = _reference()
    dataset, ds2, hw, _seed = CASES[name]
    diag, side = thresholds(dataset, ds2)
    # modules/detection.py:223-295: only the frames with labels reach the evaluator (get_valid_labels_and_batch_indices)
    lab_list, pred_list = [], []
    for n in range(labels.shape[0]):
        if counts[n] == 0:
            continue
        lab_list.append(ObjectLabels(torch.from_numpy(labels[n, :counts[n]].copy()), hw))
        pred_list.append(torch.from_numpy(det[n, :n_det[n]].copy()) if n_det[n] else None)
    gt_proph, dt_proph = to_prophesee(lab_list, pred_list)
    fn = lambda x: filter_boxes(x, int(5e5), diag, side)   # noqa: E731  (evaluation.py:33-38)
    flattened_gt, flattened_dt = [], []
    for gt_boxes, dt_boxes in zip(map(fn, gt_proph), map(fn, dt_proph)):   # coco_eval.py:42-51
        all_ts = np.unique(gt_boxes['t'])
        gt_win, dt_win = coco_eval._match_times(all_ts, gt_boxes, dt_boxes, 50000)
        flattened_gt = flattened_gt + gt_win
        flattened_dt = flattened_dt + dt_win
    categories = [{"id": i + 1, "name": str(i), "supercategory": "none"} for i in range(N_CLASSES[dataset])]
    dataset_d, results = coco_eval._to_coco_format(flattened_gt, flattened_dt, categories, height=hw[0], width=hw[1])
    ann = dataset_d["annotations"]
    f32 = lambda rows: np.asarray([[np.float32(v) for v in r] for r in rows], np.float32).reshape(-1, 4)   # noqa: E731
    for r in ann + results:
        assert all(isinstance(v, np.float32) for v in r["bbox"])
    return {
        "n_images": np.int64(len(dataset_d["images"])),
        "gt_image_id": np.asarray([a["image_id"] for a in ann], np.int64),
        "gt_category_id": np.asarray([a["category_id"] for a in ann], np.int64),
        "gt_bbox": f32([a["bbox"] for a in ann]),
        "gt_area": np.asarray([a["area"] for a in ann], np.float64),
        "gt_id": np.asarray([a["id"] for a in ann], np.int64),
        "dt_image_id": np.asarray([r["image_id"] for r in results], np.int64),
        "dt_category_id": np.asarray([r["category_id"] for r in results], np.int64),
        "dt_score": np.asarray([r["score"] for r in results], np.float64),
        "dt_bbox": f32([r["bbox"] for r in results]),
        # COCO.loadRes: ann['area'] = bb[2] * bb[3] on the np.float32 fields
        "dt_area": np.asarray([float(r["bbox"][2] * r["bbox"][3]) for r in results], np.float64),
    }


def build() -> dict:
    out = {}
    for name in CASES:
        labels, counts, det, n_det = case_inputs(name)
        out[f"{name}/labels"], out[f"{name}/counts"], out[f"{name}/det"], out[f"{name}/n_det"] = labels, counts, det, n_det
        for k, v in reference_tables(name, labels, counts, det, n_det).items():
            out[f"{name}/{k}"] = v
    return out


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {n: int(arrays[f"{n}/n_images"]) for n in CASES}, "images,",
          {n: len(arrays[f"{n}/dt_score"]) for n in CASES}, "detections")
