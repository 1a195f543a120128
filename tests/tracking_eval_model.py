"""The sequential statement of the tracking evaluator's rule (include/sast_hip.h, "tracking metrics"; sast_amd/tracking.py): one
recording at a time, frame after frame, in numpy.  The IoU is the tracker model's fp32 IoU (tests/tracker_model.py), the assignment is
`scipy.optimize.linear_sum_assignment` on the fp64 cost matrix with invalid pairs at 1e3, so the most valid pairs come first and the
least cost sum second.  Records are numpy arrays of `labels.BBOX_DTYPE`, sorted by t.

Besides the counts the model reports, per frame, what the tests need to know about their own inputs:
  margin          the uniqueness margin of the optimum: the least cost increase when one pair of the optimal assignment is forbidden
                  and the number of valid pairs stays the same (inf when no other matching has as many pairs).  The device solver sums
                  in another order than scipy, so the two may only be held to each other where this is far above rounding.
  greedy_differs  the frame's matching changes when the assignment is replaced by the tracker's greedy rule (IoU descending)
  carry_changes   the frame's matching changes when the carry-over is left out
This file IS the definition the kernel is held to, not a port of anything: parity with py-motmetrics or TrackEval is not claimed."""
import numpy as np
from scipy.optimize import linear_sum_assignment

from tracker_model import f32, iou

COLS = ("frames", "gt", "hyp", "matches", "fp", "fn", "idsw", "frag", "gt_tracks", "mt", "pt", "ml")
DIAG = ("unsorted", "refused_labels", "refused_hyp", "refused_tracks", "untracked", "bad_class", "duplicate_labels", "duplicate_hyp")
C = {name: i for i, name in enumerate(COLS)}
D = {name: i for i, name in enumerate(DIAG)}
SKIP_US = 500_000
INVALID = 1e3


def box_passes(w, h, diag2, side):
    """filter_boxes' size rule, fp32 with one rounding per operation"""
    w, h = f32(w), f32(h)
    d = f32(w * w) + f32(h * h)
    return bool(d >= f32(diag2) and w >= f32(side) and h >= f32(side))


def assign(cost_valid, ok):
    """the optimal assignment: cost_valid fp64 [n, m], ok bool [n, m] -> ({row: column} of the valid pairs, their cost sum)"""
    if 0 in ok.shape:
        return {}, 0.0
    cost = np.where(ok, cost_valid, INVALID)
    rows, cols = linear_sum_assignment(cost)
    pairs = {int(r): int(c) for r, c in zip(rows, cols) if ok[r, c]}
    return pairs, float(sum(cost[r, c] for r, c in pairs.items()))


def margin_of(cost_valid, ok, pairs, total):
    """the least cost increase over the optimum `pairs` among the matchings with as many valid pairs that leave one of its pairs out"""
    best = np.inf
    for r, c in pairs.items():
        ok2 = ok.copy()
        ok2[r, c] = False
        other, cost = assign(cost_valid, ok2)
        if len(other) == len(pairs):
            best = min(best, cost - total)
    return best


def greedy(ious, ok):
    """the tracker's rule on a frame: valid pairs by IoU descending (row, then column ascending on ties) -> {row: column}"""
    out, used = {}, set()
    for r, c in sorted(zip(*np.nonzero(ok)), key=lambda rc: (-float(ious[rc]), rc[0], rc[1])):
        if r not in out and c not in used:
            out[int(r)] = int(c)
            used.add(c)
    return out


class TrackingEvalModel:
    def __init__(self, K, min_diag2, min_side, iou_thre=0.5, time_tol_us=0, class_agnostic=False, max_gt_tracks=1024,
                 max_labels_per_frame=64, max_hyp_per_frame=128, diagnose=True):
        self.diagnose = bool(diagnose)              # False: the counts alone (no margins, no greedy / no-carry-over comparison)
        self.K, self.min_diag2, self.min_side = int(K), f32(min_diag2), f32(min_side)
        self.iou_thre, self.tol, self.agnostic = f32(iou_thre), int(time_tol_us), bool(class_agnostic)
        self.max_gt_tracks, self.max_labels, self.max_hyp = int(max_gt_tracks), int(max_labels_per_frame), int(max_hyp_per_frame)
        self.reset()

    def reset(self):
        self.acc = np.zeros((self.K + 1, len(COLS)), np.int64)
        self.acc_iou = np.zeros(self.K + 1, np.float64)
        self.acc_diag = np.zeros(len(DIAG), np.int64)

    # ---- steps 2 and 3: the records of one side of a frame
    def _side(self, rec, hyp, diag):
        """rec: the records of one label timestamp / one detection run, in order -> the indices left"""
        keep, seen = [], set()
        for i in range(len(rec)):
            if not (int(rec["t"][i]) > SKIP_US and box_passes(rec["w"][i], rec["h"][i], self.min_diag2, self.min_side)):
                continue
            if hyp and int(rec["track_id"][i]) == 0:
                diag[D["untracked"]] += 1
                continue
            if int(rec["class_id"][i]) >= self.K:
                diag[D["bad_class"]] += 1
                continue
            if int(rec["track_id"][i]) in seen:
                diag[D["duplicate_hyp" if hyp else "duplicate_labels"]] += 1
                continue
            seen.add(int(rec["track_id"][i]))
            keep.append(i)
        return rec[keep]

    def _run(self, dt, t):
        """the detection run nearest t inside the tolerance, the earlier one on a tie -> its records (before the filter)"""
        ts = np.unique(dt["t"].astype(np.int64))
        if len(ts) == 0:
            return dt[:0]
        dist = np.abs(ts - t)
        k = int(np.argmin(dist))                  # the first of equal distances: the earlier run
        if dist[k] > self.tol:
            return dt[:0]
        return dt[dt["t"] == ts[k]]

    def _pairs(self, lab, hyp):
        """-> (fp32 IoUs [n, m], valid [n, m])"""
        n, m = len(lab), len(hyp)
        if n == 0 or m == 0:
            return np.zeros((n, m), f32), np.zeros((n, m), bool)
        a = np.stack([lab["x"], lab["y"], lab["w"], lab["h"]], -1).astype(f32)
        b = np.stack([hyp["x"], hyp["y"], hyp["w"], hyp["h"]], -1).astype(f32)
        v = iou(a[:, None, :], b[None, :, :])
        with np.errstate(invalid="ignore"):
            ok = v >= self.iou_thre
        if not self.agnostic:
            ok &= lab["class_id"][:, None] == hyp["class_id"][None, :]
        return v, ok

    def _match(self, lab, hyp, last, v, ok, carry=True, solver=None):
        """step 5 -> ({label index: hypothesis index}, the margin of the assignment part)"""
        hid = [int(x) for x in hyp["track_id"]]
        match, claimed = {}, set()
        if carry:
            for o in range(len(lab)):
                h = last.get(int(lab["track_id"][o]), 0)
                if h != 0 and h in hid:
                    j = hid.index(h)
                    if j not in claimed and ok[o, j]:
                        match[o] = j
                        claimed.add(j)
        rows = [o for o in range(len(lab)) if o not in match]
        cols = [j for j in range(len(hyp)) if j not in claimed]
        sub_ok = ok[np.ix_(rows, cols)]
        sub_v = v[np.ix_(rows, cols)]
        margin = np.inf
        if solver is None:
            cost = 1.0 - sub_v.astype(np.float64)
            pairs, total = assign(cost, sub_ok)
            if self.diagnose:
                margin = margin_of(cost, sub_ok, pairs, total)
        else:
            pairs = solver(sub_v, sub_ok)
        for r, c in pairs.items():
            match[rows[r]] = cols[c]
        return match, margin

    # ---- one recording
    def recording(self, gt, dt):
        """gt, dt: BBOX_DTYPE arrays of the recording's labels and detections -> dict(rows int64 [K + 1, 12], iou fp64 [K + 1],
        diag int64 [8], frames: one dict per frame).  A refused or unsorted recording: zeros, and its reason 1 in diag."""
        K = self.K
        rows, sums, diag, frames = np.zeros((K + 1, len(COLS)), np.int64), np.zeros(K + 1, np.float64), np.zeros(len(DIAG), np.int64), []

        def refused(why):
            d = np.zeros(len(DIAG), np.int64)
            d[D[why]] = 1
            return dict(rows=np.zeros_like(rows), iou=np.zeros_like(sums), diag=d, frames=[])

        tg, td = gt["t"].astype(np.int64), dt["t"].astype(np.int64)
        if (tg[1:] < tg[:-1]).any() or (td[1:] < td[:-1]).any():
            return refused("unsorted")
        tracks, last = {}, {}             # id -> [class, present, matched, matched in the previous frame]; id -> last hypothesis id
        for t in np.unique(tg):
            lab = self._side(gt[tg == t], False, diag)
            if len(lab) == 0:
                continue
            if len(lab) > self.max_labels:
                return refused("refused_labels")
            hyp = self._side(self._run(dt, int(t)), True, diag)
            if len(hyp) > self.max_hyp:
                return refused("refused_hyp")
            for o in range(len(lab)):
                tracks.setdefault(int(lab["track_id"][o]), [int(lab["class_id"][o]), 0, 0, False])
            if len(tracks) > self.max_gt_tracks:
                return refused("refused_tracks")
            v, ok = self._pairs(lab, hyp)
            match, margin = self._match(lab, hyp, last, v, ok)
            frames.append(dict(t=int(t), n=len(lab), m=len(hyp), pairs=len(match)))
            if self.diagnose:
                frames[-1].update(margin=margin, greedy_differs=self._match(lab, hyp, last, v, ok, solver=greedy)[0] != match,
                                  carry_changes=self._match(lab, hyp, last, v, ok, carry=False)[0] != match)
            rows[:, C["frames"]] += 1
            for o in range(len(lab)):
                k, tr = int(lab["class_id"][o]), tracks[int(lab["track_id"][o])]
                rows[k, C["gt"]] += 1
                tr[1] += 1
                if o in match:
                    h = int(hyp["track_id"][match[o]])
                    rows[k, C["matches"]] += 1
                    sums[k] += float(v[o, match[o]])
                    before = last.get(int(lab["track_id"][o]), 0)
                    if before != 0 and before != h:
                        rows[k, C["idsw"]] += 1
                    if tr[2] > 0 and not tr[3]:
                        rows[k, C["frag"]] += 1
                    last[int(lab["track_id"][o])] = h
                    tr[2] += 1
                    tr[3] = True
                else:
                    rows[k, C["fn"]] += 1
                    tr[3] = False
            matched_h = set(match.values())
            for j in range(len(hyp)):
                rows[int(hyp["class_id"][j]), C["hyp"]] += 1
                if j not in matched_h:
                    rows[int(hyp["class_id"][j]), C["fp"]] += 1
        for k, present, matched, _prev in tracks.values():
            rows[k, C["gt_tracks"]] += 1
            rows[k, C["mt" if 5 * matched >= 4 * present else "ml" if 5 * matched < present else "pt"]] += 1
        frames_n = rows[0, C["frames"]]
        rows[K] = rows[:K].sum(axis=0)
        rows[K, C["frames"]] = frames_n
        for k in range(K):
            sums[K] += sums[k]
        return dict(rows=rows, iou=sums, diag=diag, frames=frames)

    def add_recordings(self, gts, dts):
        """the recordings of one call -> (rows int64 [S, K + 1, 12], iou fp64 [S, K + 1], diag int64 [S, 8], frames per recording);
        the accumulator takes them in row order"""
        out = [self.recording(g, d) for g, d in zip(gts, dts)]
        for r in out:
            self.acc += r["rows"]
            self.acc_iou += r["iou"]
            self.acc_diag += r["diag"]
        return np.stack([r["rows"] for r in out]), np.stack([r["iou"] for r in out]), np.stack([r["diag"] for r in out]), [r["frames"] for r in out]

    def evaluate(self, k=None):
        """the dict of `TrackingEvaluator.evaluate` (k: of one class) from the accumulator"""
        k = self.K if k is None else k
        out = {name: int(self.acc[k, i]) for i, name in enumerate(COLS)}

        def ratio(a, b):
            return float(a) / float(b) if b else float("nan")

        out["MOTA"] = 1.0 - ratio(out["fn"] + out["fp"] + out["idsw"], out["gt"])
        out["MOTP"] = ratio(self.acc_iou[k], out["matches"])
        out["recall"] = ratio(out["matches"], out["gt"])
        out["precision"] = ratio(out["matches"], out["matches"] + out["fp"])
        return out
