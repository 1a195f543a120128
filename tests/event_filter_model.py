"""The sequential model of `sast_amd.events.EventFilter` (csrc/k_evfilter.hip): plain Python / numpy, one event at a time, exactly the
rule of include/sast_hip.h.  Rule numbers refer to the list in INTEGRATION.md §3b "Noise filters".

One `FilterModel` is one stream row.  Nothing here is vectorised on purpose: the device decides a chunk at once, this walks it."""
import numpy as np

MODES = ("activity", "contrast")


class FilterModel:
    def __init__(self, height, width, mode="activity", threshold_us=10_000, radius=1):
        assert mode in MODES and 1 <= radius <= 3 and threshold_us >= 0
        self.height, self.width, self.mode, self.threshold_us, self.radius = height, width, mode, int(threshold_us), radius
        self.reset()
        self.err = 0

    def reset(self):
        """rule 7: the surface to -1, the carry to 0 (and the row's cumulative counts: a new recording)"""
        self.surface = np.full((self.height, self.width), -1, np.int64)
        self.t_last = 0
        self.seen = self.kept = 0

    def _recent(self, v, t):
        return v >= 0 and t - (v >> 1) <= self.threshold_us

    def push(self, x, y, p, t, reset=False):
        """one chunk in arrival order -> (x, y, p, t' of the kept events, the keep mask over the chunk)"""
        if reset:
            self.reset()
        keep = np.zeros(len(t), bool)
        tc = np.zeros(len(t), np.int64)
        H, W, r = self.height, self.width, self.radius
        for i in range(len(t)):
            xi, yi, pbit = int(x[i]), int(y[i]), int(int(p[i]) > 0)
            self.t_last = max(self.t_last, int(t[i]))                # rule 1: the running maximum, carried across calls
            tc[i] = ti = self.t_last
            self.seen += 1
            if not (0 <= xi < W and 0 <= yi < H):                    # rule 5: never passes, writes nothing, is counted; t' advanced
                self.err += 1
                continue
            if self.mode == "activity":                              # rule 3: the surface as events 0 .. i-1 left it
                for qy in range(max(yi - r, 0), min(yi + r, H - 1) + 1):
                    for qx in range(max(xi - r, 0), min(xi + r, W - 1) + 1):
                        if (qx, qy) != (xi, yi) and self._recent(int(self.surface[qy, qx]), ti):
                            keep[i] = True
            else:                                                    # rule 4
                v = int(self.surface[yi, xi])
                keep[i] = self._recent(v, ti) and (v & 1) == pbit
            self.surface[yi, xi] = 2 * ti + pbit                     # rule 2: every in-sensor event, kept or not; last by arrival order
            self.kept += int(keep[i])
        x, y, p = (np.asarray(c)[keep] for c in (x, y, p))           # rule 6: arrival order, x, y, p unchanged, t = t'
        return x, y, p, tc[keep], keep


def run(rows, height, width, cuts=(), **kw):
    """rows: one (x, y, p, t) per stream row, each cut into chunks at `cuts` (indices, clipped to the row) -> per row the concatenated
    (x, y, p, t) of the kept events, and the models (their state is the state after the recording)"""
    out, models = [], []
    for x, y, p, t in rows:
        m = FilterModel(height, width, **kw)
        edges = [0] + sorted(min(max(int(c), 0), len(t)) for c in cuts) + [len(t)]
        parts = [m.push(x[a:b], y[a:b], p[a:b], t[a:b])[:4] for a, b in zip(edges[:-1], edges[1:])]
        out.append(tuple(np.concatenate([q[k] for q in parts]) for k in range(4)))
        models.append(m)
    return out, models


def thresholds(height, width):
    """the thresholds of the randomised tests for `recording`'s event rate (a mean step of 3 us): between 0.10 and 0.90 of the events
    pass, which every randomised test asserts on the model first"""
    return {"activity": int(round(0.26 * height * width * 3)), "contrast": int(round(1.5 * height * width * 3))}


def recording(seed, n, height, width, t_start=2 ** 33 + 12345, signed_p=False):
    """n random events -> int64 x, y, p, t: x uniform in -1 .. width and y in -1 .. height (some events are outside the sensor), p in
    {0, 1} ({-1, 1} with signed_p), time steps uniform in 0 .. 6 us (ties are frequent), 5 % of the events pulled back by up to 40 us"""
    rng = np.random.RandomState(seed)
    x = rng.randint(-1, width + 1, size=n).astype(np.int64)
    y = rng.randint(-1, height + 1, size=n).astype(np.int64)
    p = rng.randint(0, 2, size=n).astype(np.int64)
    if signed_p:
        p = 2 * p - 1
    t = t_start + np.cumsum(rng.randint(0, 7, size=n)).astype(np.int64)
    back = rng.rand(n) < 0.05
    t[back] -= rng.randint(1, 41, size=int(back.sum()))
    return x, y, p, t
