"""A sequential model of sast_amd.events.Evt3Decoder and an encoder, in numpy / pure Python: Prophesee EVT 3.0, 16-bit little-endian
words with running state, by the rule of include/sast_hip.h (the table is restated in `Decoder.feed`).  The CPU tests hold the model to
the encoder (round trip) and to itself over every cut of a stream; the GPU tests compare the device decoder with it word for word."""
from __future__ import annotations

import numpy as np

ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12, VECT_8, TIME_LOW, CONTINUED_4, TIME_HIGH, EXT_TRIGGER, OTHERS, CONTINUED_12 = \
    0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x8, 0xA, 0xE, 0xF
IGNORED = (CONTINUED_4, EXT_TRIGGER, OTHERS, CONTINUED_12)          # valid words without effect
UNKNOWN = (0x1, 0x9, 0xB, 0xC, 0xD)                                 # no effect, counted
BX_CAP = 1 << 30                                                    # base_x stops growing here
STATE_FIELDS = ("y", "base_x", "vpol", "low", "high", "wraps", "have_high")


def word(type_code: int, v: int) -> int:
    assert 0 <= type_code <= 15 and 0 <= v <= 0xFFF
    return (type_code << 12) | v


class Decoder:
    """one stream: `feed(words)` -> int64 (x, y, p, t) of the chunk's events; the state and the counters carry on"""

    def __init__(self):
        self.reset()
        self.before_high = self.unknown = 0

    def reset(self):
        self.y = self.base_x = self.vpol = self.low = self.high = self.wraps = 0
        self.have_high = False

    def state(self):
        """as a row of the device's state tensor: int64 [8]"""
        return np.array([getattr(self, f) for f in STATE_FIELDS] + [0], np.int64)

    def feed(self, words):
        xs, ys, ps, ts = [], [], [], []

        def emit(x, p):
            if not self.have_high:
                self.before_high += 1
                return
            xs.append(min(x, 32767))                                # stored as int16 with saturation
            ys.append(self.y)
            ps.append(p)
            ts.append(self.wraps * (1 << 24) + self.high * 4096 + self.low)

        for w in np.asarray(words).astype(np.int64) & 0xFFFF:
            w = int(w)
            tc, v = w >> 12, w & 0xFFF
            if tc == ADDR_Y:
                self.y = v & 0x7FF
            elif tc == ADDR_X:
                emit(v & 0x7FF, v >> 11)
            elif tc == VECT_BASE_X:
                self.base_x, self.vpol = v & 0x7FF, v >> 11
            elif tc in (VECT_12, VECT_8):
                bits = 12 if tc == VECT_12 else 8
                for i in range(bits):
                    if (v >> i) & 1:
                        emit(self.base_x + i, self.vpol)
                self.base_x = min(self.base_x + bits, BX_CAP)
            elif tc == TIME_LOW:
                self.low = v
            elif tc == TIME_HIGH:
                if self.have_high and self.high - v >= 2048:
                    self.wraps += 1
                self.high, self.have_high = v, True
            elif tc in UNKNOWN:
                self.unknown += 1
        return tuple(np.array(c, np.int64) for c in (xs, ys, ps, ts))


def decode(words, cuts=()):
    """a whole stream, fed in pieces cut at the word positions `cuts` -> (x, y, p, t), (before_high, unknown), state"""
    d = Decoder()
    edges = [0] + sorted(int(c) for c in cuts) + [len(words)]
    parts = [d.feed(words[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), (d.before_high, d.unknown), d.state()


class Encoder:
    """events (t non-decreasing over all calls, 0 <= x, y <= 2047, p in 0..1) -> uint16 EVT 3.0 words that `Decoder` turns back into
    exactly them: `feed(x, y, p, t)` gives the words of one batch of events and keeps the encoder's picture of the decoder's state, so
    the batches of a recording can be encoded one by one.  Single events and, with `vectors`, VECT_12 / VECT_8 bursts for runs of events
    of one (t, y, p) with ascending x inside 12 / 8 columns; words without effect interleaved with probability `others`; TIME_HIGH
    keep-alives at most 1024 steps apart, so that every wrap of the 12-bit TIME_HIGH is seen as one."""

    def __init__(self, seed: int = 0, vectors: bool = True, others: float = 0.1):
        self.rng = np.random.RandomState(seed)
        self.vectors, self.others = vectors, others
        self.high = self.low = self.y = self.base_x = self.vpol = None      # the decoder's state (None: not set yet)
        self.last_t = 0

    def feed(self, x, y, p, t) -> np.ndarray:
        x, y, p, t = (np.asarray(c, np.int64) for c in (x, y, p, t))
        assert (np.diff(t) >= 0).all() and (len(t) == 0 or t[0] >= self.last_t)
        assert ((0 <= x) & (x <= 2047)).all() and ((0 <= y) & (y <= 2047)).all() and ((0 <= p) & (p <= 1)).all()
        rng, out = self.rng, []

        def put(w):
            out.append(w)
            if rng.rand() < self.others:
                out.append(word(IGNORED[rng.randint(len(IGNORED))], int(rng.randint(4096))))

        i, n = 0, len(t)
        while i < n:
            high, low = int(t[i]) >> 12, int(t[i]) & 0xFFF            # high: the unwrapped count of 4096 us steps
            if self.high != high:
                if self.high is None:
                    self.high = min(high, 4095)                       # the decoder starts with wraps = 0
                    put(word(TIME_HIGH, self.high))
                while high - self.high > 1024:
                    self.high += 1024
                    put(word(TIME_HIGH, self.high & 0xFFF))
                if self.high != high:
                    self.high = high
                    put(word(TIME_HIGH, self.high & 0xFFF))
            if self.low != low:
                self.low = low
                put(word(TIME_LOW, low))
            if self.y != int(y[i]):
                self.y = int(y[i])
                put(word(ADDR_Y, self.y | (int(rng.randint(2)) << 11)))   # bit 11 (master / slave) is ignored
            j = i + 1
            while self.vectors and j < n and t[j] == t[i] and y[j] == y[i] and p[j] == p[i] and x[j] > x[j - 1] and x[j] - x[i] < 12:
                j += 1
            if j - i >= 2 or (self.vectors and rng.rand() < 0.1):
                x0, pol = int(x[i]), int(p[i])
                bits = 8 if x[j - 1] - x0 < 8 and rng.rand() < 0.5 else 12
                if (self.base_x, self.vpol) != (x0, pol):
                    put(word(VECT_BASE_X, x0 | (pol << 11)))
                mask = 0
                for k in range(i, j):
                    mask |= 1 << int(x[k] - x0)
                if bits == 8:
                    mask |= int(rng.randint(16)) << 8                 # bits 8-11 of a VECT_8 are ignored
                put(word(VECT_12 if bits == 12 else VECT_8, mask))
                self.base_x, self.vpol = x0 + bits, pol
            else:
                put(word(ADDR_X, int(x[i]) | (int(p[i]) << 11)))
            i = j
        if n:
            self.last_t = int(t[-1])
        return np.array(out, np.uint16)


def encode(x, y, p, t, seed: int = 0, vectors: bool = True, others: float = 0.1) -> np.ndarray:
    """a whole recording through one `Encoder`"""
    return Encoder(seed, vectors, others).feed(x, y, p, t)


def recording(seed: int, n: int, height: int = 48, width: int = 64, t_start: int = 100, t_step: int = 40, bursts: float = 0.3,
              t_end=None):
    """n events for the encoder: non-decreasing times from t_start (mean step t_step; with t_end, spread evenly up to it instead, which
    takes the clock through wraps), single pixels and, with probability `bursts`, runs of 2 .. 6 events of one time, row and polarity
    on ascending columns -> int64 x, y, p, t"""
    rng = np.random.RandomState(seed)
    xs, ys, ps, ts = [], [], [], []
    t = t_start
    step = t_step if t_end is None else max((t_end - t_start) * 2 // max(n, 1), 1)
    while len(ts) < n:
        t += int(rng.randint(0, step + 1))
        yy, pp = int(rng.randint(height)), int(rng.randint(2))
        if rng.rand() < bursts:
            k = int(rng.randint(2, 7))
            x0 = int(rng.randint(0, max(width - 12, 1)))
            cols = x0 + np.sort(rng.choice(min(12, width - x0), size=min(k, width - x0), replace=False))
        else:
            cols = [int(rng.randint(width))]
        for c in cols:
            xs.append(int(c)), ys.append(yy), ps.append(pp), ts.append(t)
    return tuple(np.array(c[:n], np.int64) for c in (xs, ys, ps, ts))
