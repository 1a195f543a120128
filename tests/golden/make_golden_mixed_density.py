"""Fixtures of the mixed-density event stack (sast_amd.events.MixedDensityEventStack and representation="mixed_density"):
`python tests/golden/make_golden_mixed_density.py` -> mixed_density.npz.

The expected frames come from the reference itself: MixedDensityEventStack.construct of data/utils/representations.py, called on the
CPU.  The script around it (scripts/genx/preprocess_dataset.py) cannot be imported here, so its reader, window search and int8
downsampling are restated below with their line numbers, as make_golden_events.py does.  The events are not stored: they are
regenerated from that module's integer hash, so the GPU tests rebuild the same inputs without the reference.

`restatement()` is the rule the device kernels implement, in numpy, with the bin taken from the fp32 exponent.  The generator refuses
a fixture in which the reference's bin of any event differs from that rule (`reference_bins`: the reference's own construct on the same
times, one pixel per event), so no expected value depends on the last bit of a libm's logarithm.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_events as G  # noqa: E402

OUT = os.path.join(HERE, "mixed_density.npz")

H, W = 24, 72                     # three 32-column tiles, the last one partial; 12 x 36 downsampled
BINS = (3, 10, 20, 24)
CUTOFFS = (None, 10, 127, 0)

# hot pixels (x, y, permille, polarity), odd coordinates (they survive the downsampling): more than 255 net positive events (the int8
# sums wrap twice before the clamp), more than 127, net negative below -128, and -- see inputs() -- exactly balanced
HOT = ((5, 3, 100, 1), (37, 11, 45, 1), (69, 21, 50, 0), (33, 1, 40, None))
BALANCED = (33, 1)


# ---- the rule (points 1-7 of the feature's description), numpy ------------------------------------------------------------------------

def exponent_bins(t: np.ndarray, bins: int) -> np.ndarray:
    """bin of every event of one window (t sorted, non-empty): max(bins + floor(log2(t_norm)), 0) from the fp32 exponent"""
    t = np.asarray(t, np.int64)
    span = np.float32(max(int(t[-1]) - int(t[0]), 1))
    tn = (t - t[0]).astype(np.float32) / span                    # both operands rounded to fp32, one correctly rounded division
    tn = np.clip(tn, np.float32(1e-6), np.float32(1 - 1e-6))
    _m, e = np.frexp(tn)                                         # tn = m * 2^e, m in [0.5, 1)
    return np.maximum(bins + e.astype(np.int64) - 1, 0)


def restatement(x, y, p, t, bins, height, width, count_cutoff=None, downsample_by_2=False) -> np.ndarray:
    """one window -> int8 [bins, H', W']"""
    x, y, p, t = (np.asarray(a, np.int64) for a in (x, y, p, t))
    acc = np.zeros((bins, height, width), np.int64)
    if len(t):
        np.add.at(acc, (exponent_bins(t, bins), y, x), 2 * p - 1)
    acc = np.cumsum(acc, axis=0)
    acc = ((acc + 128) % 256) - 128                              # the int8 wrap
    if count_cutoff is not None:
        acc = np.clip(acc, -count_cutoff, count_cutoff)
    if downsample_by_2:
        acc = acc[:, 1::2, 1::2][:, :height // 2, :width // 2]   # nearest-exact at 0.5: output (i, j) is input (2i+1, 2j+1)
    return acc.astype(np.int8)


def window_bounds(t, ends, duration_us=None, num_events=None):
    """preprocess_dataset.py:507-512 on corrected timestamps -> [B, 2]"""
    ends = np.asarray(ends, np.int64)
    e = np.searchsorted(t, ends, side="right")
    s = np.maximum(e - num_events, 0) if num_events is not None else np.searchsorted(t, ends - duration_us, side="left")
    return np.stack([s, e], 1).astype(np.int64)


def restated_frames(x, y, p, t, kw, ends, t_carry=0):
    """the reader (time correction from the carry, polarity clip), the windows and the rule -> (frames [B, bins, H', W'], bounds)"""
    t = G.correct_time(np.asarray(t, np.int64), t_carry)
    b = window_bounds(t, ends, kw.get("duration_us"), kw.get("num_events"))
    fr = [restatement(x[s:e], y[s:e], np.clip(p[s:e], 0, None), t[s:e], kw["bins"], kw["height"], kw["width"], kw.get("count_cutoff"),
                      kw.get("downsample_by_2", False)) for s, e in b]
    return np.stack(fr), b


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def _balance(x, y, p):
    m = np.flatnonzero((x == BALANCED[0]) & (y == BALANCED[1]))
    m = m[:len(m) // 2 * 2]
    p[m] = np.arange(len(m)) % 2
    return p


def inputs(kind: str):
    """int64 x, y, p, t of a construct case"""
    if kind == "span_50000":
        x, y, p, t = G.stream(seed=71, n=4000, height=H, width=W, t_start=1000, t_span=50000, hot=HOT)
        return x, y, _balance(x, y, p), t
    if kind == "span_7":
        return G.stream(seed=72, n=3000, height=H, width=W, t_start=5, t_span=7)
    if kind == "one_event":
        return G.stream(seed=73, n=1, height=H, width=W, t_start=99)
    if kind == "two_events_same_time":
        x, y, p, t = G.stream(seed=74, n=2, height=H, width=W, t_start=99)
        t[:] = 99
        return x, y, p, t
    if kind == "ties_2p20":
        x, y, p, t = G.stream(seed=75, n=2048, height=H, width=W, t_start=0, t_span=1 << 20)
        for k in range(16, 0, -1):                                # events exactly at t_norm = 2^-k, three of each
            v = (1 << 20) >> k
            i = int(np.searchsorted(t, v))
            t[i:i + 3] = v
        assert (np.diff(t) >= 0).all() and t[0] == 0 and t[-1] == 1 << 20
        return x, y, p, t
    if kind == "empty":
        return G.stream(seed=76, n=0, height=H, width=W)
    raise KeyError(kind)


# MixedDensityEventStack.construct on one window (the whole arrays): (name, inputs kind, bins, count_cutoff)
CONSTRUCT = [(f"span_50000_b{b}_c{c}", "span_50000", b, c) for b in BINS for c in CUTOFFS]
CONSTRUCT += [(f"{k}_b{b}", k, b, None) for k in ("span_7", "one_event", "two_events_same_time", "ties_2p20") for b in (10, 24)]
CONSTRUCT += [("ties_2p20_b20_c10", "ties_2p20", 20, 10), ("empty_b10", "empty", 10, 10)]

# EventFrames(representation="mixed_density"): B = 4 overlapping windows
_STREAM = dict(seed=81, n=6000, height=H, width=W, t_start=2000, t_step=16, hot=HOT, jitter=30)
_ENDS = [9000, 21000, 26000, 47000]
BATCHED = []
for _ds in (False, True):
    BATCHED.append((f"duration_ds{int(_ds)}", dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=15000, downsample_by_2=_ds), _ENDS))
    BATCHED.append((f"count_ds{int(_ds)}", dict(height=H, width=W, bins=20, count_cutoff=None, num_events=2500, downsample_by_2=_ds), _ENDS))
EVEN_WINDOW = 1                   # this window's first and last event sit on even coordinates: the downsampling drops both

# the time-correction carry across two calls: the second chunk starts at an event whose timestamp lies below the carry (the first
# chunk's maximum), and the first count window starts with that event, so its t0 -- and with it the bins -- need the carry
_CARRY_STREAM = dict(seed=82, n=5000, height=H, width=W, t_start=0, t_step=8, jitter=400)
_CARRY_ENDS = [14000, 17000]


def _carry_case():
    t = G.stream(**_CARRY_STREAM)[3]
    tc = G.correct_time(t)
    split = 1200 + int(np.flatnonzero(t[1200:] + 100 < tc[1200:])[0])            # pulled back by more than 100 us
    n_ev = int(np.searchsorted(tc, _CARRY_ENDS[0], side="right")) - split
    return ("carry", _CARRY_STREAM, dict(height=H, width=W, bins=10, count_cutoff=127, num_events=n_ev), _CARRY_ENDS, split)


CARRY = _carry_case()

# EventStreams: S = 3 rows, T = 2, two calls; the second call resets row 1
S_CAP = 2600
S_KW = dict(height=H, width=W, bins=20, count_cutoff=10, duration_us=6000, downsample_by_2=True)
S_FIRST = [dict(seed=91, n=1500, height=H, width=W, t_start=5000, t_step=6, jitter=50),
           dict(seed=92, n=900, height=H, width=W, t_start=40000, t_step=6),
           dict(seed=93, n=1, height=H, width=W, t_start=7000)]
S_SECOND = [dict(seed=94, n=2500, height=H, width=W, t_start=8000, t_step=5, hot=HOT, jitter=50),     # starts below row 0's carry
            dict(seed=95, n=2000, height=H, width=W, t_start=100, t_step=6, jitter=20),               # a new recording: far below row 1's carry
            dict(seed=96, n=1200, height=H, width=W, t_start=7000, t_step=9)]
S_RESET = [0, 1, 0]
S_ENDS = [[11000, 3000, 9000], [13000, 5000, 11500]]           # [T, S], each on its row's own clock


def batched_inputs(kw, ends):
    """the stream with the first and last event of window EVEN_WINDOW moved to even coordinates"""
    x, y, p, t = G.stream(**_STREAM)
    p = _balance(x, y, p)
    s, e = window_bounds(G.correct_time(t), ends, kw.get("duration_us"), kw.get("num_events"))[EVEN_WINDOW]
    assert e - s > 2
    x[s], y[s], x[e - 1], y[e - 1] = 2, 4, 70, 22
    return x, y, p, t


# ---- the reference --------------------------------------------------------------------------------------------------------------------

def downsample_int8(r):
    """preprocess_dataset.py:463-473, int8 branch: + 128 as uint8, nearest-exact at 0.5, - 128 back to int8"""
    import torch
    u = (r.to(torch.int16) + 128).to(torch.uint8)
    u = torch.nn.functional.interpolate(u.unsqueeze(0), scale_factor=0.5, mode="nearest-exact")[0]
    d = (u.to(torch.int16) - 128).to(torch.int8)
    assert torch.equal(d, r[:, 1::2, 1::2])
    return d


def reference_bins(rep_mod, t, bins):
    """the reference's bin of every event: its own construct on the same times, event i alone on pixel (0, i) with polarity 1 -- channel c
    of that pixel is 1 from the event's bin on"""
    import torch
    n = len(t)
    rep = rep_mod.MixedDensityEventStack(bins=bins, height=1, width=n)
    r = rep.construct(torch.arange(n), torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64), torch.from_numpy(np.asarray(t, np.int64)))
    return bins - r[:, 0, :].to(torch.int64).sum(0).numpy()


def reference_construct(rep_mod, x, y, p, t, bins, height, width, cutoff):
    import torch
    if len(t):
        want, got = exponent_bins(t, bins), reference_bins(rep_mod, t, bins)
        assert np.array_equal(want, got), f"the reference's bin differs from the exponent rule for {int((want != got).sum())} events"
    rep = rep_mod.MixedDensityEventStack(bins=bins, height=height, width=width, count_cutoff=cutoff)
    return rep.construct(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), torch.from_numpy(p.copy()), torch.from_numpy(t.copy()))


def reference_frames(rep_mod, x, y, p, t, kw, ends, t_carry=0):
    """preprocess_dataset.py:476-530 on in-memory arrays -> (frames [B, bins, H', W'] int8, bounds [B, 2])"""
    t = G.correct_time(t, t_carry)
    b = window_bounds(t, ends, kw.get("duration_us"), kw.get("num_events"))
    frames = []
    for s, e in b:
        r = reference_construct(rep_mod, x[s:e], y[s:e], np.clip(p[s:e], 0, None), t[s:e], kw["bins"], kw["height"], kw["width"],
                                kw.get("count_cutoff"))
        if kw.get("downsample_by_2"):
            r = downsample_int8(r)
        frames.append(r.numpy())
    return np.stack(frames), b


def generate() -> dict:
    rep_mod = G.load_representations()
    out = {}
    for name, kind, bins, cut in CONSTRUCT:
        x, y, p, t = inputs(kind)
        out[f"construct/{name}"] = reference_construct(rep_mod, x, y, p, t, bins, H, W, cut).numpy()
    for name, kw, ends in BATCHED:
        x, y, p, t = batched_inputs(kw, ends)
        frames, bounds = reference_frames(rep_mod, x, y, p, t, kw, ends)
        s, e = bounds[EVEN_WINDOW]
        assert x[s] % 2 == 0 and y[s] % 2 == 0 and x[e - 1] % 2 == 0 and y[e - 1] % 2 == 0
        assert (bounds[1:, 0] < bounds[:-1, 1]).any() and (bounds[:, 1] > bounds[:, 0]).all(), "overlapping, non-empty windows"
        out[f"batched/{name}/frames"] = frames
        out[f"batched/{name}/bounds"] = bounds
    name, skw, kw, ends, split = CARRY
    x, y, p, t = G.stream(**skw)
    frames, bounds = reference_frames(rep_mod, x, y, p, t, kw, ends)
    assert (bounds[:, 0] >= split).all() and bounds[0, 0] == split and 1000 < split < 2000
    assert not np.array_equal(restated_frames(x[split:], y[split:], p[split:], t[split:], kw, ends)[0], frames), "the carry must matter"
    out[f"batched/{name}/frames"] = frames
    out[f"batched/{name}/bounds"] = bounds
    first = [G.stream(**k) for k in S_FIRST]
    second = [G.stream(**k) for k in S_SECOND]
    fr, bd, last = [], [], []
    for s, (a, b) in enumerate(zip(first, second)):
        carry = 0 if S_RESET[s] else int(G.correct_time(a[3]).max())
        f, bnd = reference_frames(rep_mod, *b, S_KW, [row[s] for row in S_ENDS], t_carry=carry)
        fr.append(f)
        bd.append(bnd)
        last.append(int(G.correct_time(b[3], carry).max()))
    out["streams/frames"] = np.stack(fr, 1)                       # [T, S, bins, H', W']
    out["streams/bounds"] = np.stack(bd, 1)                       # [T, S, 2], row-local
    out["streams/t_last"] = np.array(last, np.int64)
    assert all(int(np.count_nonzero(f)) for f in out["streams/frames"].reshape(-1, *fr[0].shape[1:]))
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
