"""A sequential model of sast_amd.events.Evt2Encoder in numpy / pure Python: events -> Prophesee EVT 2.0 / EVT 2.1 words by the canonical
rule of include/sast_hip.h (restated in `Encoder.feed`).  One event after the other, with the decoder's time base in plain variables:
the CPU tests hold it to `evt2_model.Decoder` (round trip), the GPU tests compare the device encoder with it word for word.  The word
builders are those of evt2_model.py; its randomised `Encoder` is another thing (it interleaves words without effect and picks vector
bases at random): this one is deterministic."""
from __future__ import annotations

import numpy as np

import evt2_model as M

STATE_FIELDS = ("have", "t_last")
MAX_XY = 2047
KEEP_STEPS = 1 << 26                                                 # two neighbouring TIME_HIGHs are at most this far apart


def keep_alives(t_prev: int, t: int) -> int:
    """TIME_HIGH words sent only to keep two neighbours at most 2^26 steps apart"""
    gap = (t >> 6) - (t_prev >> 6)
    return (gap - 1) // KEEP_STEPS if gap > 0 else 0


class Encoder:
    """one stream: `feed(x, y, p, t)` -> the uint32 (2.0) / uint64 (2.1) words of the chunk; the state (have, t_last) and the counters
    carry on"""

    def __init__(self, version: str):
        assert version in M.VERSIONS
        self.version = version
        self.reset()
        self.raised = self.clamped = self.refused = 0

    def reset(self):
        self.have, self.t_last = False, 0

    def state(self):
        """as a row of the device's state tensor: int64 [4]"""
        return np.array([int(self.have), self.t_last, 0, 0], np.int64)

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
        n, ver = len(t), self.version
        out = []

        def cont(j):                                                 # event j continues the group of event j - 1 (EVT 2.1 only)
            return (ver == M.V21 and 0 < j < n and t[j] == t[j - 1] and y[j] == y[j - 1] and p[j] == p[j - 1] and x[j - 1] < x[j]
                    and x[j - 1] >> 5 == x[j] >> 5)

        have, t_prev = self.have, self.t_last
        i = 0
        while i < n:
            ti, yi, xi, pi = int(t[i]), int(y[i]), int(x[i]), int(p[i])
            j = i + 1
            while cont(j):
                j += 1
            assert j - i <= 32
            if not have:
                out.append(M.time_high(ver, (ti >> 6) & M.HIGH_MASK))
            elif ti >> 6 > t_prev >> 6:
                for q in range(1, keep_alives(t_prev, ti) + 1):
                    out.append(M.time_high(ver, ((t_prev >> 6) + KEEP_STEPS * q) & M.HIGH_MASK))
                out.append(M.time_high(ver, (ti >> 6) & M.HIGH_MASK))
            if ver == M.V20:
                out.append(M.cd(ver, pi, ti & 63, xi, yi))
            else:
                valid = 0
                for k in range(i, j):
                    valid |= 1 << int(x[k] & 31)
                out.append(M.cd(ver, pi, ti & 63, 32 * (xi >> 5), yi, valid))
            have, t_prev = True, ti                                  # the members of a group share the leader's time
            i = j
        if max_words is not None and len(out) > max_words:           # refused whole: nothing changes but the counter
            self.refused += 1
            return M.array(ver, [])
        if n:
            self.have, self.t_last = True, t_prev
        self.raised += raised
        self.clamped += clamped
        return M.array(ver, out)


def encode(x, y, p, t, version: str, cuts=()):
    """a whole recording through one `Encoder`, fed in chunks cut at the event positions `cuts` -> the words of every chunk, one after
    the other"""
    enc = Encoder(version)
    edges = [0] + sorted(int(c) for c in cuts) + [len(t)]
    parts = [enc.feed(*(c[a:b] for c in (x, y, p, t))) for a, b in zip(edges[:-1], edges[1:])]
    return np.concatenate(parts) if parts else M.array(version, [])
