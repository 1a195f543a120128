"""A sequential model of sast_amd.events.Evt3Encoder in numpy / pure Python: events -> Prophesee EVT 3.0 words by the canonical rule of
include/sast_hip.h (restated in `Encoder.feed`).  One event after the other, with the decoder's state in plain variables: the CPU tests
hold it to `evt3_model.Decoder` (round trip), the GPU tests compare the device encoder with it word for word."""
from __future__ import annotations

import numpy as np

import evt3_model as M

STATE_FIELDS = ("have", "t_last", "y_last")
MAX_XY = 2047


def keep_alives(t_prev: int, t: int) -> int:
    """TIME_HIGH words sent only to keep two neighbours at most 1024 steps apart"""
    gap = (t >> 12) - (t_prev >> 12)
    return (gap - 1) // 1024 if gap > 0 else 0


class Encoder:
    """one stream: `feed(x, y, p, t)` -> the uint16 words of the chunk; the state (have, t_last, y_last) and the counters carry on"""

    def __init__(self):
        self.reset()
        self.raised = self.clamped = self.refused = 0

    def reset(self):
        self.have, self.t_last, self.y_last = False, 0, 0

    def state(self):
        """as a row of the device's state tensor: int64 [4]"""
        return np.array([int(self.have), self.t_last, self.y_last, 0], np.int64)

    def normalise(self, x, y, p, t):
        """the running maximum of t from the row's carry (0 for a new recording), x and y clamped to 0 .. 2047, p != 0; nothing is
        dropped -> the four columns, the events whose time was raised, the events whose x, y or p was changed"""
        x, y, p, t = (np.asarray(c, np.int64) for c in (x, y, p, t))
        seed = self.t_last if self.have else 0
        tn = np.maximum.accumulate(np.concatenate([[seed], t]))[1:] if len(t) else t
        xn, yn, pn = np.clip(x, 0, MAX_XY), np.clip(y, 0, MAX_XY), (p != 0).astype(np.int64)
        return (xn, yn, pn, tn), int((tn != t).sum()), int(((xn != x) | (yn != y) | (pn != p)).sum())

    def feed(self, x, y, p, t, max_words=None) -> np.ndarray:
        (x, y, p, t), raised, clamped = self.normalise(x, y, p, t)
        n = len(t)
        out = []

        def cont(j):                                                 # event j continues the group of event j - 1
            return (0 < j < n and t[j] == t[j - 1] and y[j] == y[j - 1] and p[j] == p[j - 1] and x[j - 1] < x[j]
                    and x[j - 1] // 12 == x[j] // 12)

        have, t_prev, y_prev = self.have, self.t_last, self.y_last
        i = 0
        while i < n:
            ti, yi, xi, pi = int(t[i]), int(y[i]), int(x[i]), int(p[i])
            j = i + 1
            while cont(j):
                j += 1
            high = False
            if not have:
                out.append(M.word(M.TIME_HIGH, (ti >> 12) & 0xFFF))
                high = True
            else:
                for q in range(1, keep_alives(t_prev, ti) + 1):
                    out.append(M.word(M.TIME_HIGH, ((t_prev >> 12) + 1024 * q) & 0xFFF))
                if ti >> 12 != t_prev >> 12:
                    out.append(M.word(M.TIME_HIGH, (ti >> 12) & 0xFFF))
                    high = True
            if high or (ti & 0xFFF) != (t_prev & 0xFFF):
                out.append(M.word(M.TIME_LOW, ti & 0xFFF))
            if not have or yi != y_prev:
                out.append(M.word(M.ADDR_Y, yi))
            if j - i >= 2:
                chained = (i >= 2 and cont(i - 1) and t[i - 1] == ti and y[i - 1] == yi and p[i - 1] == pi and x[i - 1] < xi
                           and xi // 12 == x[i - 1] // 12 + 1)
                if not chained:
                    out.append(M.word(M.VECT_BASE_X, 12 * (xi // 12) | (pi << 11)))
                mask = 0
                for k in range(i, j):
                    mask |= 1 << int(x[k] % 12)
                out.append(M.word(M.VECT_12, mask))
            else:
                out.append(M.word(M.ADDR_X, xi | (pi << 11)))
            have, t_prev, y_prev = True, int(t[j - 1]), yi
            i = j
        if max_words is not None and len(out) > max_words:           # refused whole: nothing changes but the counter
            self.refused += 1
            return np.zeros(0, np.uint16)
        if n:
            self.have, self.t_last, self.y_last = True, t_prev, y_prev
        self.raised += raised
        self.clamped += clamped
        return np.array(out, np.uint16)


def encode(x, y, p, t, cuts=()):
    """a whole recording through one `Encoder`, fed in chunks cut at the event positions `cuts` -> the words of every chunk, one after
    the other"""
    enc = Encoder()
    edges = [0] + sorted(int(c) for c in cuts) + [len(t)]
    parts = [enc.feed(*(c[a:b] for c in (x, y, p, t))) for a, b in zip(edges[:-1], edges[1:])]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint16)
