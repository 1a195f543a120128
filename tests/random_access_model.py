"""A numpy model of sast_amd.sampling.RandomAccessPool on top of the rows of label_streams_model.py: the item index of
SequenceForRandomAccess.__init__ (data/genx_utils/sequence_rnd.py:24-35) and torch's ConcatDataset, the windows and labels of
__getitem__ (:43-60), get_most_recent_objframe (data/utils/augmentor.py:367-378) and the weights of get_weighted_random_sampler
(data/genx_utils/dataset_rnd.py:115-149), restated with Python integers and numpy's fp64 operations, plus the status bits and the
out-of-range rule the device class adds.  The CPU tests pin it to the fixture the reference's own classes wrote
(tests/golden/random_access.npz); the GPU tests use it at the batches the fixture does not hold."""
from __future__ import annotations

import bisect

import numpy as np

CLASS_ID, ITEM_INDEX = 1, 2          # status bits (sast_amd.sampling, include/sast_hip.h): per row, pool-wide


class Pool:
    def __init__(self, rows, sequence_length: int, only_load_end_labels: bool = False, max_classes: int = 16):
        """rows: label_streams_model.Row, one per recording (a flagged row has no frames)"""
        self.rows, self.L, self.only_end, self.max_classes = list(rows), int(sequence_length), bool(only_load_end_labels), int(max_classes)
        self.start_idx_offset, self.length = [], []
        for r in self.rows:
            off = r.n_frames
            for j, w in enumerate(r.frame_2_window.tolist()):
                if w - self.L + 1 >= 0:
                    off = j
                    break
            self.start_idx_offset.append(off)
            self.length.append(r.n_frames - off)
        self.cum = [0]
        for n in self.length:
            self.cum.append(self.cum[-1] + n)
        self.N = self.cum[-1]
        self.status = [0] * len(self.rows)
        self.pool_status = 0

    def locate(self, g: int):
        """ConcatDataset.__getitem__: item -> (row, label frame, start_idx, end_idx), or None outside [0, N)"""
        if not 0 <= g < self.N:
            return None
        r = bisect.bisect_right(self.cum[1:], g)
        j = g - self.cum[r] + self.start_idx_offset[r]
        end = int(self.rows[r].frame_2_window[j]) + 1
        assert end - self.L >= 0
        return r, j, end - self.L, end

    def step_frames(self, g: int):
        """per step of item g the label frame its window holds, or None (no label frame, or a step only_load_end_labels leaves out)"""
        r, _j, start, end = self.locate(g)
        row = self.rows[r]
        out = []
        for w in range(start, end):
            f = int(row.window_2_frame[w])
            out.append(None if f < 0 or (self.only_end and w < end - 1) else f)
        return r, out

    def frame_rows(self, r: int, f: int) -> np.ndarray:
        row = self.rows[r]
        o, n = int(row.frame_start[f]), int(row.frame_count[f])
        return row.labels[o:o + n]

    def batch(self, items, M: int):
        """-> rows, window_idx, ends_us, labels, counts, labelled, latest, latest_count as RandomAccessPool.batch gives them"""
        B, L = len(items), self.L
        rows = np.full(B, -1, np.int32)
        widx, ends = np.full((L, B), -1, np.int64), np.full((L, B), -1, np.int64)
        labels, counts, labelled = np.zeros((L, B, M, 7), np.float32), np.zeros((L, B), np.int32), np.zeros((L, B), np.uint8)
        latest, latest_count = np.zeros((B, M, 7), np.float32), np.zeros(B, np.int32)
        for b, g in enumerate(int(v) for v in items):
            loc = self.locate(g)
            if loc is None:
                self.pool_status |= ITEM_INDEX
                continue
            r, _j, start, end = loc
            rows[b] = r
            _r, frames = self.step_frames(g)
            for k, f in enumerate(frames):
                widx[k, b], ends[k, b] = start + k, self.rows[r].ends_us[start + k]
                if f is None:
                    continue
                lab = self.frame_rows(r, f)
                labelled[k, b], counts[k, b] = 1, len(lab)
                labels[k, b, :len(lab)] = lab
            for k in range(L - 1, -1, -1):              # reversed(sparse_obj_labels): the first one that is not None and not empty
                if counts[k, b] > 0:
                    latest_count[b] = counts[k, b]
                    latest[b] = labels[k, b]
                    break
        return rows, widx, ends, labels, counts, labelled, latest, latest_count

    def item_class_counts(self, g: int) -> np.ndarray:
        r, frames = self.step_frames(g)
        cnt = np.zeros(self.max_classes, np.int64)
        for f in frames:
            if f is None:
                continue
            for c in self.frame_rows(r, f)[:, 5].tolist():
                if 0 <= c < self.max_classes:
                    cnt[int(c)] += 1
                else:
                    self.status[r] |= CLASS_ID
        return cnt

    def weights(self):
        """-> class_total int64 [max_classes], weights fp64 [N]"""
        per_item = [self.item_class_counts(g) for g in range(self.N)]
        total = np.sum(per_item, axis=0, dtype=np.int64) if per_item else np.zeros(self.max_classes, np.int64)
        out = np.zeros(self.N, np.float64)
        for g, cnt in enumerate(per_item):
            w = np.float64(0.0)
            for c in range(self.max_classes):
                if cnt[c]:
                    w = w + (np.float64(1.0) / np.float64(max(int(total[c]), 1))) * np.float64(cnt[c])
            out[g] = w
        return total, out

    def labelled_pairs(self, items) -> int:
        K = 0
        for g in items:
            if self.locate(int(g)) is not None:
                K += sum(f is not None for f in self.step_frames(int(g))[1])
        return K
