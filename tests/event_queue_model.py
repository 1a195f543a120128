"""A numpy model of sast_amd.events.EventQueue: the same storage, heads, counts, carries, retirement records and error counters, one row
at a time.  The CPU tests hold it to whole-recording window bounds over random chunkings; the GPU tests compare device state with it.

Beside the device's state the model keeps, per row, `origin`: the number (within the recording) of the event in storage slot 0, so a
storage index is turned into an event identity that does not depend on chunking or compaction."""
from __future__ import annotations

import numpy as np

DURATION, COUNT = 0, 1


def decode_dat(records: np.ndarray):
    """int32 / uint32 [..., 2] Event2D records -> int64 x, y, p, t, by the masks of the reference's load_td_data
    (utils/evaluation/prophesee/io/dat_events_tools.py:39-50): t unsigned, bits 29-31 of word 1 ignored"""
    w = np.ascontiguousarray(records).view(np.uint32).astype(np.int64)
    return w[..., 1] & 16383, (w[..., 1] >> 14) & 16383, (w[..., 1] >> 28) & 1, w[..., 0]


def encode_dat(x, y, p, t, high_bits=0) -> np.ndarray:
    """-> int32 [n, 2] records; high_bits (0 .. 7) goes to bits 29-31 of word 1"""
    w1 = (np.asarray(x, np.int64) & 16383) | ((np.asarray(y, np.int64) & 16383) << 14) | ((np.asarray(p, np.int64) & 1) << 28) \
        | ((np.asarray(high_bits, np.int64) & 7) << 29)
    return np.stack([np.asarray(t, np.int64) & 0xFFFFFFFF, w1], -1).astype(np.uint32).view(np.int32)


class QueueModel:
    def __init__(self, S: int, capacity: int, mode: int, value: int):
        self.S, self.cap, self.mode, self.value = S, capacity, mode, value
        self.x, self.y, self.p = (np.zeros((S, capacity), np.int16) for _ in range(3))
        self.t = np.zeros((S, capacity), np.int64)
        self.head, self.count, self.t_last, self.retired, self.retired_t, self.origin = (np.zeros(S, np.int64) for _ in range(6))
        self.err = np.zeros(4, np.int64)
        self.moves, self.moves_skipped = np.zeros(S, np.int64), np.zeros(S, np.int64)

    def reset_row(self, s):
        for v in (self.head, self.count, self.t_last, self.retired, self.retired_t, self.origin):
            v[s] = 0

    def push(self, rows, reset=None):
        """rows: per row (x, y, p, t) int64 arrays of the chunk's valid events (timestamps as read: int64, or the unsigned word)"""
        for s, (x, y, p, t) in enumerate(rows):
            if reset is not None and reset[s]:
                self.reset_row(s)
            c = int(self.count[s])
            n = min(len(t), self.cap - c)
            self.err[2] += len(t) - n
            tc = np.maximum.accumulate(np.concatenate([[self.t_last[s]], np.asarray(t[:n], np.int64)]))
            self.t[s, c:c + n] = tc[1:]
            for dst, src in ((self.x, x), (self.y, y), (self.p, p)):
                dst[s, c:c + n] = np.clip(np.asarray(src[:n], np.int64), -32768, 32767)
            self.t_last[s] = tc[-1]
            self.count[s] = c + n

    def frames(self, ends):
        """ends [T, S] -> (bounds [T, S, 2] as row-relative storage indices, the same as event identities: bounds + origin at the time
        of the search), then the retirement"""
        ends = np.asarray(ends, np.int64).reshape(-1, self.S)
        bounds = np.zeros(ends.shape + (2,), np.int64)
        for s in range(self.S):
            h, c = int(self.head[s]), int(self.count[s])
            live = self.t[s, h:c]
            for k in range(ends.shape[0]):
                e = h + int(np.searchsorted(live, ends[k, s], side="right"))
                if self.mode == COUNT:
                    b = max(e - self.value, h)
                    late = e - h < self.value and self.retired[s] > 0
                else:
                    b = h + int(np.searchsorted(live, ends[k, s] - self.value, side="left"))
                    late = self.retired[s] > 0 and self.retired_t[s] >= ends[k, s] - self.value
                self.err[3] += int(late)
                bounds[k, s] = (b, e)
        ident = bounds + self.origin[None, :, None]
        for s in range(self.S):
            h, c, start = int(self.head[s]), int(self.count[s]), int(bounds[-1, s, 0])
            if start > h:
                self.retired[s] += start - h
                self.retired_t[s] = self.t[s, start - 1]
            live = c - start
            if start > 0 and live <= start:
                for a in (self.x, self.y, self.p, self.t):
                    a[s, :live] = a[s, start:c].copy()
                self.head[s], self.count[s] = 0, live
                self.origin[s] += start
                self.moves[s] += 1
            else:
                self.head[s] = start
                self.moves_skipped[s] += int(start > 0)
        return bounds, ident


def whole_bounds(t, ends, mode, value):
    """the windows of a whole recording (preprocess_dataset.py:507-513 on corrected timestamps): [T, 2] event numbers"""
    tc = np.maximum.accumulate(np.concatenate([[0], np.asarray(t, np.int64)]))[1:]
    ends = np.asarray(ends, np.int64)
    e = np.searchsorted(tc, ends, side="right")
    b = np.maximum(e - value, 0) if mode == COUNT else np.searchsorted(tc, ends - value, side="left")
    return np.stack([b, e], 1)


def schedule(times, seed: int, max_chunk: int, value: int, steps=(1, 2, 3), tail: int = 2):
    """a streaming session over S recordings (times: their raw timestamps) that honours EventQueue's contract: a list of rounds
    (cuts [S, 2]: the events [lo, hi) each row pushes; ends [T, S]: the window ends asked for after the push).  Every end is below the
    corrected time of the row's last pushed event unless the recording is over, ends never decrease, and the last step of a round asks
    for the latest end the row may give, so a row retains about one window.  `tail` rounds follow the last push."""
    rng = np.random.RandomState(seed)
    S = len(times)
    tc = [np.maximum.accumulate(np.concatenate([[0], np.asarray(t, np.int64)]))[1:] for t in times]
    pushed, prev = [0] * S, [0] * S
    rounds = []
    left = tail
    while left > 0:
        if all(pushed[s] == len(tc[s]) for s in range(S)):
            left -= 1
        T = int(steps[rng.randint(len(steps))])
        cuts, ends = np.zeros((S, 2), np.int64), np.zeros((T, S), np.int64)
        for s in range(S):
            n = len(tc[s])
            hi = min(n, pushed[s] + int(rng.randint(0, max_chunk + 1)))
            cuts[s] = (pushed[s], hi)
            pushed[s] = hi
            if hi == n:
                top = (int(tc[s][-1]) if n else 0) + value // 2 + 1 if prev[s] <= (int(tc[s][-1]) if n else 0) else prev[s]
            else:
                top = int(tc[s][hi - 1]) - 1 if hi else prev[s]
            top = max(top, prev[s])
            mids = np.sort(rng.randint(prev[s], top + 1, size=T - 1)) if T > 1 else []
            ends[:, s] = list(mids) + [top]
            prev[s] = top
        rounds.append((cuts, ends))
    return rounds
