"""A plain-Python model of sast_amd.online: the window scheduler (sast_evq_schedule) and the bookkeeping of one push step.

The scheduler is written from its definition, one window at a time, not from the kernel's closed form: window k of a call ends at
e_k = next_end + k * D and is due when an event later than e_k was pushed (t_last > e_k), or, for a recording that is over, while the
window still holds an event time (e_k - D < t_last)."""
from __future__ import annotations

import numpy as np


class SchedulerModel:
    def __init__(self, S: int, D: int, W: int, first_end: int = None):
        self.S, self.D, self.W = S, int(D), int(W)
        self.first_end = self.D if first_end is None else int(first_end)
        assert self.D >= 1 and self.first_end >= self.D
        self.next_end = np.full(S, self.first_end, np.int64)

    def is_due(self, e: int, t_last: int, final: bool) -> bool:
        return t_last > e or (final and e - self.D < t_last)

    def step(self, t_last, reset=None, final=None):
        """t_last [S]: the queue's carry after the push -> ends [W, S], due [W, S] (uint8), backlog [S]; next_end advances"""
        S, D, W = self.S, self.D, self.W
        ends, due, backlog = np.zeros((W, S), np.int64), np.zeros((W, S), np.uint8), np.zeros(S, np.int64)
        for s in range(S):
            if reset is not None and reset[s]:
                self.next_end[s] = self.first_end
            ne, tl, fin = int(self.next_end[s]), int(t_last[s]), bool(final is not None and final[s])
            n = 0
            while n < W and self.is_due(ne + n * D, tl, fin):
                n += 1
            more = 0
            while self.is_due(ne + (n + more) * D, tl, fin):
                more += 1
            for k in range(W):
                ends[k, s] = ne + k * D if k < n else ne + (n - 1) * D
                due[k, s] = k < n
            backlog[s] = more
            self.next_end[s] = ne + n * D
        return ends, due, backlog


class StepModel:
    """one push of OnlineDetector on the host: the carries of the time correction (the queue's t_last), then the schedule.  The callers
    keep the recordings; this keeps what the device keeps."""

    def __init__(self, S: int, D: int, W: int, first_end: int = None):
        self.sched = SchedulerModel(S, D, W, first_end)
        self.t_last = np.zeros(S, np.int64)

    def push(self, times, reset=None, final=None):
        """times: per row the raw timestamps of the chunk -> (ends, due, backlog) of the step"""
        for s, t in enumerate(times):
            if reset is not None and reset[s]:
                self.t_last[s] = 0
            if len(t):
                self.t_last[s] = max(int(self.t_last[s]), int(np.max(t)))
        return self.sched.step(self.t_last, reset, final)


def to_prophesee_records(det: np.ndarray, t: int, dtype) -> np.ndarray:
    """the detection half of to_prophesee on one frame's rows (x1, y1, x2, y2, obj_conf, class_conf, class_pred), numpy fp32 arithmetic"""
    det = np.asarray(det, np.float32).reshape(-1, 7)
    out = np.zeros(len(det), dtype=dtype)
    out['t'] = t
    out['x'], out['y'] = det[:, 0], det[:, 1]
    out['w'], out['h'] = det[:, 2] - det[:, 0], det[:, 3] - det[:, 1]
    out['class_id'] = det[:, 6].astype(np.uint32)
    out['class_confidence'] = det[:, 5]
    return out
