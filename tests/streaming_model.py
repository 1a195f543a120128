"""A numpy model of sast_amd.sampling.StreamingPool on top of the rows of label_streams_model.py: the sub-sequences of
_get_ev_repr_range_indices / SequenceForIter.get_sequences_with_guaranteed_labels (data/genx_utils/sequence_for_streaming.py:21-50,
86-111), the samples and the padded tail of SequenceForIter.__init__ / __getitem__ (:53-84, 137-181), get_fully_padded_sample
(:120-132), the deals of ShardedStreamingDataPipe (data/utils/stream_sharded_datapipe.py:19-67), restated with Python integers, plus
the cursor, the status bits and the bad-entry rule the device class adds.  The CPU tests pin it to the fixture the reference's own
classes wrote (tests/golden/streaming.npz); the GPU tests use it at the schedules the fixture does not hold."""
from __future__ import annotations

import numpy as np

TRUNCATED, SCHEDULE_INDEX = 1, 2          # status bits (sast_amd.sampling, include/sast_hip.h): pool-wide

NAMES = ("rows", "step_rows", "seq", "sample", "is_first", "exhausted", "window_idx", "ends_us", "labels", "counts", "labelled",
         "is_padded")


def row_sequences(f2w, n_windows: int, L: int, guarantee_labels: bool):
    """the (start, stop) window ranges of one recording, in ascending window order"""
    f2w = [int(v) for v in f2w]
    if not f2w:
        return []                         # a flagged row: the reference would crash on objframe_idx_2_repr_idx[0]
    if not guarantee_labels:
        return [(max(f2w[0] - L + 1, 0), n_windows)]
    out, a = [], 0
    for j in range(1, len(f2w) + 1):
        if j == len(f2w) or f2w[j] - f2w[j - 1] > L:
            out.append((max(f2w[a] - L + 1, 0), f2w[j - 1] + 1))
            a = j
    return out


def pyramid(n: int):
    while True:
        yield from range(n)
        yield from range(n - 1, -1, -1)


class Pool:
    def __init__(self, rows, sequence_length: int, guarantee_labels: bool = True, max_sequences=None):
        """rows: label_streams_model.Row, one per recording (a flagged row has no frames)"""
        self.rows, self.L, self.guarantee = list(rows), int(sequence_length), bool(guarantee_labels)
        self.status = 0
        seqs, self.row_first_seq = [], [0]
        for r, row in enumerate(self.rows):
            for start, stop in row_sequences(row.frame_2_window, row.n_windows, self.L, self.guarantee):
                seqs.append((r, start, stop, -(-(stop - start) // self.L)))
            self.row_first_seq.append(len(seqs))
        if max_sequences is not None and len(seqs) > max_sequences:
            self.status |= TRUNCATED
            seqs = seqs[:max_sequences]
            self.row_first_seq = [min(v, max_sequences) for v in self.row_first_seq]
        self.sequences = np.asarray(seqs, np.int32).reshape(-1, 4)
        self.n_seq = len(seqs)
        self.orders, self.cursor = None, None

    # ---- one sample
    def sample(self, s: int, i: int):
        """-> row, the windows of the L steps (None: padded)"""
        r, start, stop, samples = (int(v) for v in self.sequences[s])
        assert 0 <= i < samples
        lo = start + i * self.L
        return r, [w if w < stop else None for w in range(lo, lo + self.L)]

    def step_frame(self, r: int, w):
        """the label frame of window w of row r, or None"""
        if w is None:
            return None
        f = int(self.rows[r].window_2_frame[w])
        return None if f < 0 else f

    # ---- schedules
    def sharded_orders(self, batch_size: int, total_num_workers: int = 1, global_worker_id: int = 0):
        samples = self.sequences[:, 3].tolist()
        if not len(samples) >= total_num_workers > global_worker_id:
            raise ValueError("workers")
        ids = sorted(range(len(samples)), key=lambda s: samples[s], reverse=True)
        mine = [s for s, w in zip(ids, pyramid(total_num_workers)) if w == global_worker_id]
        if len(mine) < batch_size:
            raise ValueError("batch_size")
        mine = sorted(mine, key=lambda s: samples[s], reverse=True)
        out = [[] for _ in range(batch_size)]
        for s, b in zip(mine, pyramid(batch_size)):
            out[b].append(s)
        return out

    def set_schedule(self, orders):
        self.orders = [[int(s) for s in o] for o in orders]
        self.cursor = [[0, 0] for _ in self.orders]

    def walk(self):
        """per batch row the (sequence, sample) of every step; a bad entry is one step (None, None)"""
        out = []
        for o in self.orders:
            w = []
            for s in o:
                if not 0 <= s < self.n_seq:
                    w.append((None, None))
                else:
                    w.extend((s, i) for i in range(int(self.sequences[s, 3])))
            out.append(w)
        return out

    def steps(self, mode: str) -> int:
        n = [len(w) for w in self.walk()]
        return min(n) if mode == "shortest" else max(n)

    def plan(self):
        walk = self.walk()
        n, B = max(len(w) for w in walk), len(walk)
        K, first, seq = np.zeros(n, np.int64), np.zeros((n, B), bool), np.full((n, B), -1, np.int32)
        for b, w in enumerate(walk):
            for step, (s, i) in enumerate(w):
                r, windows = self.sample(s, i)
                K[step] += sum(self.step_frame(r, x) is not None for x in windows)
                first[step, b], seq[step, b] = i == 0, s
        return K, first, seq

    def next(self, M: int):
        """-> the twelve arrays of a StreamingBatch, and the cursors move on"""
        B, L = len(self.orders), self.L
        rows, seq, sample = (np.full(B, -1, np.int32) for _ in range(3))
        is_first, exhausted = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
        step_rows = np.full((L, B), -1, np.int32)
        widx, ends = np.full((L, B), -1, np.int64), np.full((L, B), -1, np.int64)
        labels, counts = np.zeros((L, B, M, 7), np.float32), np.zeros((L, B), np.int32)
        labelled, padded = np.zeros((L, B), np.uint8), np.ones((L, B), np.uint8)
        for b, o in enumerate(self.orders):
            pos, i = self.cursor[b]
            if pos >= len(o):
                exhausted[b] = 1
                continue
            s = o[pos]
            if not 0 <= s < self.n_seq:
                self.status |= SCHEDULE_INDEX
                self.cursor[b] = [pos + 1, 0]
                continue
            r, windows = self.sample(s, i)
            rows[b], seq[b], sample[b], is_first[b] = r, s, i, i == 0
            row = self.rows[r]
            for k, w in enumerate(windows):
                if w is None:
                    continue
                step_rows[k, b], widx[k, b], ends[k, b], padded[k, b] = r, w, row.ends_us[w], 0
                f = self.step_frame(r, w)
                if f is not None:
                    o_, n_ = int(row.frame_start[f]), int(row.frame_count[f])
                    labelled[k, b], counts[k, b] = 1, n_
                    labels[k, b, :n_] = row.labels[o_:o_ + n_]
            self.cursor[b] = [pos, i + 1] if i + 1 < int(self.sequences[s, 3]) else [pos + 1, 0]
        return rows, step_rows, seq, sample, is_first, exhausted, widx, ends, labels, counts, labelled, padded
