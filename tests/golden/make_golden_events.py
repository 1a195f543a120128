"""Fixtures of the raw-events front end (sast_amd/events.py): `python tests/golden/make_golden_events.py` -> events.npz.

The expected frames come from the reference itself: StackedHistogram.construct of data/utils/representations.py, imported from the
reference root that `_ref_import.py` names (that module imports only numpy and torch).  The offline script around it,
scripts/genx/preprocess_dataset.py, cannot be imported without h5py / numba / hydra, so its reader and windowing are restated below
with their line numbers.

The events are not stored: `stream()` regenerates them from a small integer hash (no library RNG stream), so the GPU tests rebuild the
same inputs without the reference.  Small frames are stored whole; full-size batched frames as the sha256 of their bytes plus crops.
"""
from __future__ import annotations

import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "events.npz")

_M64 = (1 << 64) - 1


def _hash(seed: int, n: int, salt: int) -> np.ndarray:
    """splitmix64 of (seed, salt, index): n uint64 values"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x1000193 + salt * 0x9E3779B1) & _M64)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def stream(seed, n, height, width, t_start=0, t_step=8, hot=(), jitter=0, t_span=None):
    """n events: uniform pixels and polarities, timestamps rising by 0 .. t_step-1 per event (or spread evenly over t_span), a share
    hot[k] = (x, y, permille, pol) of them moved to hot pixels, and with jitter > 0 one event in 16 pulled back by up to `jitter` us
    (the unsorted timestamps the reader's time correction fixes).  -> int64 x, y, p, t"""
    x = (_hash(seed, n, 1) % np.uint64(width)).astype(np.int64)
    y = (_hash(seed, n, 2) % np.uint64(height)).astype(np.int64)
    p = (_hash(seed, n, 3) & np.uint64(1)).astype(np.int64)
    if t_span is not None:
        t = t_start + (np.arange(n, dtype=np.int64) * t_span) // max(n - 1, 1)
    else:
        t = t_start + np.cumsum((_hash(seed, n, 4) % np.uint64(t_step)).astype(np.int64))
    sel = (_hash(seed, n, 5) % np.uint64(1000)).astype(np.int64)
    lo = 0
    for hx, hy, permille, hp in hot:
        m = (sel >= lo) & (sel < lo + permille)
        x[m], y[m] = hx, hy
        if hp is not None:
            p[m] = hp
        lo += permille
    if jitter:
        back = (_hash(seed, n, 6) % np.uint64(16) == 0) & (np.arange(n) > 0)
        t[back] -= (_hash(seed, n, 7)[back] % np.uint64(jitter)).astype(np.int64)
        t = np.maximum(t, 0)
    return x, y, p, t


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

# StackedHistogram.construct on one window (the whole arrays): (name, stream kwargs, (bins, height, width, count_cutoff, fastmode))
_SMALL = dict(seed=11, n=60000, height=48, width=80, t_step=5, hot=((17, 9, 700, 1), (40, 30, 10, None)))   # ~42 000 / ~600 events
CONSTRUCT = [("gen1_full", dict(seed=3, n=200000, height=240, width=304, t_step=3, hot=((101, 77, 3, None), (7, 200, 2, 0))),
              (10, 240, 304, 10, True))]
for _bins in (1, 10):
    for _cut in (None, 10, 255):
        for _fast in (True, False):
            CONSTRUCT.append((f"small_b{_bins}_c{_cut}_f{int(_fast)}", _SMALL, (_bins, 48, 80, _cut, _fast)))
CONSTRUCT += [
    ("span_2p25", dict(seed=5, n=4000, height=16, width=32, t_span=(1 << 25) + 7), (10, 16, 32, None, True)),
    ("equal_times", dict(seed=6, n=3000, height=16, width=32, t_step=1), (10, 16, 32, 10, True)),
    ("empty", dict(seed=7, n=0, height=16, width=32), (10, 16, 32, 10, True)),
]


def construct_inputs(kw):
    x, y, p, t = stream(**kw)
    if kw.get("t_span") is not None:
        # the fp32 rounding at the last bin: an event at t0 + 2^25 + 1 over a span of 2^25 + 7 
        t[len(t) // 2:len(t) // 2 + 8] = t[len(t) // 2 - 1]
        t[-2] = (1 << 25) + 1
        t = np.maximum.accumulate(t)
    if kw["seed"] == 6:
        t[:] = 123456     # t1 == t0: every event in bin 0
    return x, y, p, t


# EventFrames over one buffer: (name, stream kwargs, frame kwargs, window ends in us, chunk split or None)
BATCHED = [
    ("gen4_ds2_duration", dict(seed=21, n=400000, height=720, width=1280, t_start=1000, t_step=2, hot=((641, 359, 4, None), (640, 358, 3, None)),
                               jitter=40),
     dict(height=720, width=1280, bins=10, count_cutoff=10, duration_us=50000, downsample_by_2=True), [900, 51000, 101000, 151000], None),
    ("gen4_ds2_count", dict(seed=21, n=400000, height=720, width=1280, t_start=1000, t_step=2, hot=((641, 359, 4, None), (640, 358, 3, None)),
                            jitter=40),
     dict(height=720, width=1280, bins=10, count_cutoff=10, num_events=50000, downsample_by_2=True), [900, 30000, 101000, 201000], None),
    ("gen1_duration_i16", dict(seed=22, n=150000, height=240, width=304, t_start=0, t_step=3, hot=((5, 5, 3, 1),), jitter=20),
     dict(height=240, width=304, bins=10, count_cutoff=None, fastmode=False, duration_us=50000), [50000, 100000, 150000], None),
    ("gen1_carry", dict(seed=23, n=120000, height=240, width=304, t_start=0, t_step=4, jitter=300),
     dict(height=240, width=304, bins=10, count_cutoff=10, duration_us=40000), [150000, 200000], 60000),
]
CROPS = ((0, 0), (96, 128), (200, 288))   # (top, left) of 32 x 32 crops of every channel, clipped to the frame


def crops(frames: np.ndarray) -> np.ndarray:
    """[B, C, H, W] -> [B, len(CROPS), C, 32, 32] (zero past the frame)"""
    B, C, H, W = frames.shape
    out = np.zeros((B, len(CROPS), C, 32, 32), np.uint8)
    for k, (r, c) in enumerate(CROPS):
        r, c = min(r, max(H - 32, 0)), min(c, max(W - 32, 0))
        blk = frames[:, :, r:r + 32, c:c + 32]
        out[:, k, :, :blk.shape[2], :blk.shape[3]] = blk
    return out


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the reference -------------------------------------------------------------------------------------------------------------------

def load_representations():
    sys.path.insert(0, HERE)
    import _ref_import as RI
    path = os.path.join(RI.REF_ROOT, "data", "utils", "representations.py")
    spec = importlib.util.spec_from_file_location("_ref_representations", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def correct_time(t: np.ndarray, carry: int = 0) -> np.ndarray:
    """preprocess_dataset.py:159-168 (H5Reader._correct_time): time_last starts at 0; t[i] < time_last -> time_last, else it becomes
    the new time_last -- a running maximum from the carry"""
    return np.maximum.accumulate(np.concatenate([[carry], t]))[1:]


def reference_frames(rep_mod, x, y, p, t, frame_kw, ends, t_carry=0):
    """preprocess_dataset.py:476-530 on in-memory arrays; returns (frames [B, C, H', W'] uint8, corrected t, bounds [B, 2])"""
    import torch
    t = correct_time(t, t_carry)
    ends = np.asarray(ends, np.int64)
    end_idx = np.searchsorted(t, ends, side="right")                                     # :507
    if frame_kw.get("num_events") is not None:
        start_idx = np.maximum(end_idx - frame_kw["num_events"], 0)                      # :508-509
    else:
        start_idx = np.searchsorted(t, ends - frame_kw["duration_us"], side="left")       # :511-512 (dt_ms * 1000)
    rep = rep_mod.StackedHistogram(bins=frame_kw.get("bins", 10), height=frame_kw["height"], width=frame_kw["width"],
                                   count_cutoff=frame_kw.get("count_cutoff", 10), fastmode=frame_kw.get("fastmode", True))
    frames = []
    for s, e in zip(start_idx, end_idx):
        # get_event_slice, :170-186: int64 columns, p clipped at 0
        sl = slice(int(s), int(e))
        r = rep.construct(x=torch.from_numpy(x[sl].copy()), y=torch.from_numpy(y[sl].copy()),
                          pol=torch.from_numpy(np.clip(p[sl], 0, None)), time=torch.from_numpy(t[sl].copy()))
        if frame_kw.get("downsample_by_2"):                                                # :519-522, downsample_ev_repr :463-473
            r = torch.nn.functional.interpolate(r.unsqueeze(0), scale_factor=0.5, mode="nearest-exact")[0]
        frames.append(r.numpy())
    return np.stack(frames), t, np.stack([start_idx, end_idx], 1)


def generate() -> dict:
    import torch
    rep_mod = load_representations()
    out = {}
    for name, kw, (bins, h, w, cut, fast) in CONSTRUCT:
        x, y, p, t = construct_inputs(kw)
        rep = rep_mod.StackedHistogram(bins=bins, height=h, width=w, count_cutoff=cut, fastmode=fast)
        r = rep.construct(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(p), torch.from_numpy(t))
        out[f"construct/{name}"] = r.numpy()
    for name, kw, fkw, ends, split in BATCHED:
        x, y, p, t = stream(**kw)
        frames, tc, bounds = reference_frames(rep_mod, x, y, p, t, fkw, ends)
        if split is not None:
            assert (bounds[:, 0] >= split).all(), "carry case: every window must start in the second chunk"
        out[f"batched/{name}/sha256"] = np.array(sha256(frames))
        out[f"batched/{name}/crops"] = crops(frames)
        out[f"batched/{name}/bounds"] = bounds.astype(np.int64)
        out[f"batched/{name}/t_sha256"] = np.array(sha256(tc.astype(np.int64)))
        out[f"batched/{name}/nonzero"] = np.array([int(np.count_nonzero(f)) for f in frames], np.int64)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
