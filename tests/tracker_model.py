"""The sequential statement of the tracker's rule (include/sast_hip.h, "track ids"; sast_amd/tracking.py): a plain loop in numpy fp32,
one operation per line, the total order done by sorting the candidate list.  `TrackerModel.step` is one online step over the rows,
`TrackerModel.run` the recording driver; records are numpy arrays of `labels.BBOX_DTYPE` and are changed in place (their track_id only).
The reference has no tracker: this file IS the definition the kernel is held to, not a port of anything."""
import numpy as np

f32 = np.float32


def iou(a, b):
    """a, b: fp32 arrays [..., 4] of (x, y, w, h), broadcast against each other -> fp32 [...]; every line is one fp32 operation per
    element, np.minimum / np.maximum give NaN when either side is NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        ax, ay, aw, ah = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
        bx, by, bw, bh = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
        ax2 = ax + aw
        ay2 = ay + ah
        bx2 = bx + bw
        by2 = by + bh
        lo_x = np.maximum(ax, bx)
        hi_x = np.minimum(ax2, bx2)
        iw = np.maximum(f32(0), hi_x - lo_x)
        lo_y = np.maximum(ay, by)
        hi_y = np.minimum(ay2, by2)
        ih = np.maximum(f32(0), hi_y - lo_y)
        inter = iw * ih
        area_a = aw * ah
        area_b = bw * bh
        uni = (area_a + area_b) - inter
        q = inter / uni
        out = np.where(uni > 0, q, f32(0))
    assert out.dtype == f32
    return out


def candidates(slots, dets, iou_thre, class_agnostic):
    """slots: [(i, box, cls)], dets: [(j, box, cls)] -> [(iou, j, i)] of the pairs that pass the class gate and the threshold"""
    if not slots or not dets:
        return []
    v = iou(np.array([b for _i, b, _c in slots], f32)[:, None, :], np.array([b for _j, b, _c in dets], f32)[None, :, :])
    scls = np.array([int(c) & 0xffffffff for _i, _b, c in slots], np.int64)      # the 32 bits of the class word
    dcls = np.array([int(c) for _j, _b, c in dets], np.int64)
    ok = (v >= f32(iou_thre)) & (class_agnostic or (scls[:, None] == dcls[None, :]))
    return [(v[a, b], dets[b][0], slots[a][0]) for a, b in zip(*np.nonzero(ok))]


def greedy(cands):
    """the strict total order (IoU descending, detection ascending, slot ascending), first remaining pair first -> {j: i}"""
    match, used = {}, set()
    for _v, j, i in sorted(cands, key=lambda c: (-float(c[0]), c[1], c[2])):
        if j not in match and i not in used:
            match[j] = i
            used.add(i)
    return match


class TrackerModel:
    def __init__(self, num_streams, max_det, max_tracks=64, iou_thre=0.3, max_age_us=200_000, new_score_thre=0.0, class_agnostic=False):
        S, T = num_streams, max_tracks
        self.S, self.T, self.max_det = S, T, max_det
        self.iou_thre, self.max_age_us, self.new_score_thre, self.class_agnostic = f32(iou_thre), int(max_age_us), f32(new_score_thre), class_agnostic
        self.ids = np.zeros((S, T), np.int32)
        self.box = np.zeros((S, T, 4), np.float32)
        self.cls = np.zeros((S, T), np.int32)
        self.last_t = np.zeros((S, T), np.int64)
        self.hits = np.zeros((S, T), np.int32)
        self.next_id = np.ones(S, np.int32)
        self.counters = np.zeros(4, np.int32)

    def state(self):
        return dict(ids=self.ids, box=self.box, cls=self.cls, last_t=self.last_t, hits=self.hits, next_id=self.next_id, counters=self.counters)

    def _free(self, s, i):
        self.ids[s, i] = 0
        self.box[s, i] = 0
        self.cls[s, i] = 0
        self.last_t[s, i] = 0
        self.hits[s, i] = 0

    def reset_row(self, s):
        for i in range(self.T):
            self._free(s, i)
        self.next_id[s] = 1

    def step_row(self, s, rec, t):
        """steps 3 .. 7 on rec (a BBOX_DTYPE array of m <= max_det records, changed in place) at time t"""
        t, m = int(t), len(rec)
        assert m <= self.max_det
        for i in range(self.T):                                            # 3: expire
            if self.ids[s, i] != 0 and t - int(self.last_t[s, i]) > self.max_age_us:
                self._free(s, i)
        live_before = {int(self.ids[s, i]) for i in range(self.T) if self.ids[s, i] != 0}
        slots = [(i, self.box[s, i].copy(), self.cls[s, i]) for i in range(self.T) if self.ids[s, i] != 0]
        dets = [(j, (rec["x"][j], rec["y"][j], rec["w"][j], rec["h"][j]), rec["class_id"][j]) for j in range(m)]
        match = greedy(candidates(slots, dets, self.iou_thre, self.class_agnostic))      # 4, 5
        for j, i in match.items():
            self.box[s, i] = dets[j][1]
            self.last_t[s, i] = t
            self.hits[s, i] += 1
            rec["track_id"][j] = self.ids[s, i]
        for j in range(m):                                                 # 6: births, in index order
            if j in match:
                continue
            rec["track_id"][j] = 0
            if not f32(rec["class_confidence"][j]) >= self.new_score_thre:
                continue
            free = [i for i in range(self.T) if self.ids[s, i] == 0]
            if not free:
                self.counters[0] += 1
                continue
            i = free[0]
            self.ids[s, i] = self.next_id[s]
            self.next_id[s] += 1
            self.hits[s, i] = 1
            self.box[s, i] = dets[j][1]
            self.cls[s, i] = np.uint32(dets[j][2]).astype(np.int32)
            self.last_t[s, i] = t
            rec["track_id"][j] = self.ids[s, i]
        return live_before, match

    def step(self, records, counts, ends, due, reset=None):
        """records: one BBOX_DTYPE array [max_det] per row (changed in place), counts / ends / due / reset: per row"""
        for s in range(self.S):
            if reset is not None and reset[s]:
                self.reset_row(s)
            if not due[s]:
                continue
            m = min(max(int(counts[s]), 0), self.max_det)
            self.step_row(s, records[s][:m], ends[s])

    def run(self, records, n):
        """records: one BBOX_DTYPE array [Dcap] per row (changed in place), n per row"""
        for s in range(self.S):
            self.reset_row(s)
            k = min(max(int(n[s]), 0), len(records[s]))
            t = records[s]["t"][:k].astype(np.int64)
            if (t[1:] < t[:-1]).any():
                self.counters[2] += 1
                continue
            pos = 0
            while pos < k:
                end = pos
                while end < k and t[end] == t[pos]:
                    end += 1
                m = min(end - pos, self.max_det)
                self.step_row(s, records[s][pos:pos + m], t[pos])
                if end - pos > m:
                    records[s]["track_id"][pos + m:end] = 0
                    self.counters[1] += 1
                pos = end
