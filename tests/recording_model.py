"""A plain numpy model of `PropheseeEvaluator.add_recordings` (sast_amd/evaluation.py): whole recordings as sorted `BBOX_DTYPE` records
-> filter_boxes -> the unique label timestamps -> the +-tol windows of _match_times -> the flattened tables of _to_coco_format, in the
form tests/coco_reference.py takes.  tests/golden/eval_recordings.npz pins the windows to the reference's own _match_times and
filter_boxes (tests/golden/make_golden_eval_recordings.py); this file needs neither the reference nor a GPU.

The detections of an image are found the way the device finds them: two binary searches over the UNFILTERED sorted detections, the
filter applied inside the window.  That equals the reference's two-pointer walk over the filtered detections (the fixture test)."""
import numpy as np

BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})
FIELDS = BBOX_DTYPE.names
SKIP_US = 500000


def records(n=0):
    """n zeroed records (np.zeros: the four padding bytes are zero too)"""
    return np.zeros(n, dtype=BBOX_DTYPE)


def words(rec):
    """records -> int32 [n, 10], the form the device takes"""
    if rec.dtype != BBOX_DTYPE:           # np.concatenate packs a structured dtype (36 bytes): back into the 40-byte layout, by field
        new = records(len(rec))
        for f in FIELDS:
            new[f] = rec[f]
        rec = new
    return np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), 10)


def from_words(w):
    return np.ascontiguousarray(w, dtype=np.int32).reshape(-1).view(BBOX_DTYPE)


def same_records(a, b):
    """field by field: numpy leaves a record's padding bytes undefined when it copies structured arrays"""
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def passes(rec, diag, side):
    """filter_boxes (io/box_filtering.py:31-36) on fp32 fields"""
    w, h = rec['w'].astype(np.float32), rec['h'].astype(np.float32)
    return (rec['t'] > SKIP_US) & (w * w + h * h >= np.float32(diag ** 2)) & (w >= np.float32(side)) & (h >= np.float32(side))


def is_sorted(rec):
    return bool(np.all(rec['t'][1:] >= rec['t'][:-1]))


def windows(gt, dt, tol, diag, side):
    """one recording -> a list of images (t, label indices, detection indices, records in the window before the filter)"""
    gp, dp = passes(gt, diag, side), passes(dt, diag, side)
    out = []
    for t in np.unique(gt['t'][gp]):
        lo, hi = int(np.searchsorted(dt['t'], t - tol, side='left')), int(np.searchsorted(dt['t'], t + tol, side='right'))
        out.append((int(t), np.nonzero(gp & (gt['t'] == t))[0], lo + np.nonzero(dp[lo:hi])[0], hi - lo))
    return out


class Model:
    """the buffer of one evaluator: add_recordings / add_images append, tables() is what `PropheseeEvaluator.tables()` returns"""

    def __init__(self, diag, side, max_images=1 << 30, max_detections=1 << 30, max_labels=1 << 30):
        self.diag, self.side = diag, side
        self.caps = (max_images, max_detections, max_labels)
        self.image_t, self.gt, self.dt = [], [], []       # gt rows (image id, record), dt rows (image id, record)
        self.refused = {"max_images": 0, "max_detections": 0, "max_labels_per_frame": 0, "max_window_detections": 0, "unsorted": 0}

    def add_image(self, t, g, d):
        if len(g) > self.caps[2]:
            self.refused["max_labels_per_frame"] += 1
        elif len(self.image_t) >= self.caps[0]:
            self.refused["max_images"] += 1
        elif len(self.dt) + len(d) > self.caps[1]:
            self.refused["max_detections"] += 1
        else:
            self.image_t.append(t)
            i = len(self.image_t)
            self.gt += [(i, r) for r in g]
            self.dt += [(i, r) for r in d]

    def add_recordings(self, rows, tol=50000, max_window=1024):
        """rows: a list of (gt records, dt records)"""
        for gt, dt in rows:
            if not (is_sorted(gt) and is_sorted(dt)):
                self.refused["unsorted"] += 1
                continue
            for t, gi, di, n_window in windows(gt, dt, tol, self.diag, self.side):
                if n_window > max_window:
                    self.refused["max_window_detections"] += 1
                else:
                    self.add_image(t, gt[gi], dt[di])

    def tables(self):
        def col(rows, f, dtype):
            return np.asarray([r[f] for _i, r in rows], dtype=dtype)

        def box(rows):
            return np.asarray([[r[f] for f in ('x', 'y', 'w', 'h')] for _i, r in rows], dtype=np.float32).reshape(-1, 4)
        gb, db = box(self.gt), box(self.dt)
        return {
            "image_t": np.asarray(self.image_t, dtype=np.int64),
            "gt_image_id": np.asarray([i for i, _r in self.gt], dtype=np.int64),
            "gt_category_id": col(self.gt, 'class_id', np.int64) + 1,
            "gt_bbox": gb, "gt_area": (gb[:, 2] * gb[:, 3]).astype(np.float64),
            "dt_image_id": np.asarray([i for i, _r in self.dt], dtype=np.int64),
            "dt_category_id": col(self.dt, 'class_id', np.int64) + 1,
            "dt_score": col(self.dt, 'class_confidence', np.float32),
            "dt_bbox": db, "dt_area": (db[:, 2] * db[:, 3]).astype(np.float64),
        }


def coco_inputs(tab):
    """tables -> (n_images, gt, dt) of tests/coco_reference.py"""
    gt = {"image_id": tab["gt_image_id"], "category_id": tab["gt_category_id"], "bbox": tab["gt_bbox"], "area": tab["gt_area"]}
    dt = {"image_id": tab["dt_image_id"], "category_id": tab["dt_category_id"], "bbox": tab["dt_bbox"], "area": tab["dt_area"],
          "score": tab["dt_score"].astype(np.float64)}
    return len(tab["image_t"]), gt, dt
