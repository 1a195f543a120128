"""A sequential model of sast_amd.events.Evt2Decoder and an encoder, in numpy / pure Python: Prophesee EVT 2.0 (32-bit little-endian
words, one word at most one event) and EVT 2.1 (64-bit little-endian words, one word a 32-pixel vector), by the rule of
include/sast_hip.h (the tables are restated in `Decoder.feed`).  The only running state is the time base.  The CPU tests hold the model
to the encoder (round trip) and to itself over every cut of a stream; the GPU tests compare the device decoder with it word for word.
Parity with the Metavision SDK's decoder is unpinned: this model is what is pinned."""
from __future__ import annotations

import numpy as np

V20, V21 = "2.0", "2.1"
VERSIONS = (V20, V21)
CD_OFF, CD_ON, TIME_HIGH, EXT_TRIGGER, OTHERS, CONTINUED = 0x0, 0x1, 0x8, 0xA, 0xE, 0xF
IGNORED = (EXT_TRIGGER, OTHERS, CONTINUED)                          # valid words without effect
UNKNOWN = (0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x9, 0xB, 0xC, 0xD)        # no effect, counted
HIGH_BITS, HIGH_MASK, WRAP_STEP = 28, (1 << 28) - 1, 1 << 27
STATE_FIELDS = ("high", "wraps", "have_high")
WORD_BITS = {V20: 32, V21: 64}
WORD_DTYPE = {V20: np.uint32, V21: np.uint64}
FANOUT = {V20: 1, V21: 32}                                          # the events one word can give


def word(version: str, type_code: int, payload: int = 0) -> int:
    """a word of `type_code` with the low bits `payload`"""
    bits = WORD_BITS[version] - 4
    assert 0 <= type_code <= 15 and 0 <= payload < (1 << bits)
    return (type_code << bits) | payload


def time_high(version: str, v: int) -> int:
    assert 0 <= v <= HIGH_MASK
    return word(version, TIME_HIGH, v if version == V20 else v << 32)


def cd(version: str, p: int, ts6: int, x: int, y: int, valid: int = 1) -> int:
    """an event word: EVT 2.0 CD_OFF / CD_ON of pixel (x, y); EVT 2.1 EVT_NEG / EVT_POS of row y from column x on with the mask `valid`"""
    assert p in (0, 1) and 0 <= ts6 <= 63 and 0 <= x <= 2047 and 0 <= y <= 2047
    if version == V20:
        return word(version, p, (ts6 << 22) | (x << 11) | y)
    assert 0 <= valid <= 0xFFFFFFFF
    return word(version, p, (ts6 << 54) | (x << 43) | (y << 32) | valid)


def array(version: str, words) -> np.ndarray:
    return np.array([int(w) for w in words], dtype=WORD_DTYPE[version])


class Decoder:
    """one stream: `feed(words)` -> int64 (x, y, p, t) of the chunk's events; the state and the counters carry on"""

    def __init__(self, version: str):
        assert version in VERSIONS
        self.version = version
        self.reset()
        self.before_high = self.unknown = 0

    def reset(self):
        self.high = self.wraps = 0
        self.have_high = False

    def state(self):
        """as a row of the device's state tensor: int64 [4]"""
        return np.array([getattr(self, f) for f in STATE_FIELDS] + [0], np.int64)

    def feed(self, words):
        xs, ys, ps, ts = [], [], [], []
        wide = self.version == V21
        shift = WORD_BITS[self.version] - 4
        for w in np.asarray(words).astype(WORD_DTYPE[self.version]).tolist():
            tc = w >> shift
            if tc <= CD_ON:
                if wide:
                    ts6, x0, y, valid = (w >> 54) & 0x3F, (w >> 43) & 0x7FF, (w >> 32) & 0x7FF, w & 0xFFFFFFFF
                else:
                    ts6, x0, y, valid = (w >> 22) & 0x3F, (w >> 11) & 0x7FF, w & 0x7FF, 1
                if not valid:
                    continue
                if not self.have_high:
                    self.before_high += bin(valid).count("1")
                    continue
                t = self.wraps * (1 << 34) + self.high * 64 + ts6
                while valid:                                          # the set bits, ascending
                    low = valid & -valid
                    xs.append(x0 + low.bit_length() - 1)              # up to 2047 + 31: stored as written
                    ys.append(y)
                    ps.append(tc)
                    ts.append(t)
                    valid ^= low
            elif tc == TIME_HIGH:
                v = ((w >> 32) if wide else w) & HIGH_MASK
                if self.have_high and self.high - v >= WRAP_STEP:
                    self.wraps += 1
                self.high, self.have_high = v, True
            elif tc in UNKNOWN:
                self.unknown += 1
        return tuple(np.array(c, np.int64) for c in (xs, ys, ps, ts))


def decode(words, version: str, cuts=()):
    """a whole stream, fed in pieces cut at the word positions `cuts` -> (x, y, p, t), (before_high, unknown), state"""
    d = Decoder(version)
    edges = [0] + sorted(int(c) for c in cuts) + [len(words)]
    parts = [d.feed(words[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), (d.before_high, d.unknown), d.state()


class Encoder:
    """events (t non-decreasing over all calls, 0 <= x, y <= 2047, p in 0..1) -> EVT 2.0 (uint32) or EVT 2.1 (uint64) words that
    `Decoder` turns back into exactly them: `feed(x, y, p, t)` gives the words of one batch of events and keeps the encoder's picture
    of the decoder's time base, so the batches of a recording can be encoded one by one.  TIME_HIGH wherever t >> 6 changes, with
    keep-alives at most 2^26 steps apart, so that every wrap of the 28-bit field is seen as one; words without effect interleaved with
    probability `others`.  For 2.1, runs of events of one (t, y, p) with ascending x inside 32 columns go into one word, whose base is
    the first column or (half of the time, where the run still fits) that column rounded down to a multiple of 32, as a sensor aligns
    it."""

    def __init__(self, version: str, seed: int = 0, others: float = 0.1):
        assert version in VERSIONS
        self.version, self.others = version, others
        self.rng = np.random.RandomState(seed)
        self.high = None                                              # the unwrapped count of 64 us steps (None: not set yet)
        self.last_t = 0

    def feed(self, x, y, p, t) -> np.ndarray:
        x, y, p, t = (np.asarray(c, np.int64) for c in (x, y, p, t))
        assert (np.diff(t) >= 0).all() and (len(t) == 0 or t[0] >= self.last_t)
        assert ((0 <= x) & (x <= 2047)).all() and ((0 <= y) & (y <= 2047)).all() and ((0 <= p) & (p <= 1)).all()
        rng, out, ver = self.rng, [], self.version

        def put(w):
            out.append(w)
            if rng.rand() < self.others:
                out.append(word(ver, IGNORED[rng.randint(len(IGNORED))], int(rng.randint(1 << 28))))

        i, n = 0, len(t)
        while i < n:
            high, ts6 = int(t[i]) >> 6, int(t[i]) & 0x3F
            if self.high != high:
                if self.high is None:
                    self.high = min(high, HIGH_MASK)                  # the decoder starts with wraps = 0
                    put(time_high(ver, self.high))
                while high - self.high > (1 << 26):
                    self.high += 1 << 26
                    put(time_high(ver, self.high & HIGH_MASK))
                if self.high != high:
                    self.high = high
                    put(time_high(ver, self.high & HIGH_MASK))
            j = i + 1
            if ver == V20:
                put(cd(ver, int(p[i]), ts6, int(x[i]), int(y[i])))
            else:
                while j < n and t[j] == t[i] and y[j] == y[i] and p[j] == p[i] and x[j] > x[j - 1] and x[j] - x[i] < 32:
                    j += 1
                x0 = int(x[i])
                if x[j - 1] - (x0 & ~31) < 32 and rng.rand() < 0.5:
                    x0 &= ~31
                valid = 0
                for k in range(i, j):
                    valid |= 1 << int(x[k] - x0)
                put(cd(ver, int(p[i]), ts6, x0, int(y[i]), valid))
            i = j
        if n:
            self.last_t = int(t[-1])
        return array(ver, out)


def encode(x, y, p, t, version: str, seed: int = 0, others: float = 0.1) -> np.ndarray:
    """a whole recording through one `Encoder`"""
    return Encoder(version, seed, others).feed(x, y, p, t)
