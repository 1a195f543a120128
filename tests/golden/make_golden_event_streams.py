"""Fixtures of the batched event front end (sast_amd.events.EventStreams): `python tests/golden/make_golden_event_streams.py` ->
event_streams.npz.

S recordings side by side are S independent runs of the reference: its StackedHistogram.construct behind the reader and windowing
restated in make_golden_events.py (`reference_frames`), once per recording, each with its own time-correction carry.  The events are
regenerated from `stream()`'s integer hash, so the GPU tests rebuild the same rows without the reference.  Frames are small (48 x 80
sensor) and stored whole, corrected timestamps as the sha256 of their int64 bytes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_events import correct_time, load_representations, reference_frames, sha256, stream  # noqa: E402

OUT = os.path.join(HERE, "event_streams.npz")

H, W, CAP = 48, 80, 6000          # three 32-column tiles, the last one partial; 24 x 40 with downsample_by_2
_GEO = dict(height=H, width=W)

# ---- four recordings in one call: 5 000, 0, 1 and 777 events.  Rows 2 and 3 start below row 0's last timestamps (~7 700 us), so a
# running maximum that leaks across a row boundary raises them.
ROWS = [
    dict(seed=31, n=5000, t_start=200, t_step=4, hot=((17, 9, 200, 1), (70, 40, 20, None)), jitter=60, **_GEO),
    dict(seed=32, n=0, **_GEO),
    dict(seed=33, n=1, t_start=700, t_step=4, **_GEO),
    dict(seed=34, n=777, t_start=100, t_step=4, hot=((33, 47, 100, 0),), jitter=60, **_GEO),
]
# frame kwargs and window ends [T][S] (us, each on its own recording's clock)
DURATION_KW = dict(bins=10, count_cutoff=10, duration_us=3000, **_GEO)
DURATION_ENDS = [[3000, 1000, 500, 50],         # row 2, row 3: before the recording's first event
                 [9000, 5000, 2000, 900]]       # row 0, row 2: after its last
COUNT_KW = dict(bins=10, count_cutoff=10, num_events=300, downsample_by_2=True, **_GEO)
COUNT_ENDS = [[3000, 1000, 500, 400],           # row 3: ~200 events so far, the window stops at the start of the row
              [9000, 5000, 2000, 5000]]         # row 2: its one event, the window stops at the start of the row

# ---- carry and reset over two calls.  (call 1 rows, call 2 rows): rows 0 and 3 continue their recording (split in two), row 1 has
# nothing new in call 2, row 2 starts a new recording in call 2 (reset) whose clock is far below the old one's.
_C0 = dict(seed=41, n=5000, t_start=0, t_step=4, jitter=400, **_GEO)
_C1 = dict(seed=42, n=300, t_start=20, t_step=4, jitter=30, **_GEO)
_C2_OLD = dict(seed=43, n=400, t_start=50000, t_step=4, jitter=50, **_GEO)
_C2_NEW = dict(seed=44, n=600, t_start=0, t_step=4, jitter=100, **_GEO)
_C3 = dict(seed=45, n=777, t_start=100, t_step=4, jitter=400, **_GEO)
CARRY_SPLIT = [2496, 300, None, 300]            # (rows 0, 3: call 2 begins with an event below the carry) events of the recording fed by call 1 (row 2: all of the old recording)
CARRY_KW = dict(bins=10, count_cutoff=10, duration_us=500, **_GEO)
CARRY_ENDS = [[4500, 100, 400, 1150],
              [7400, 200, 1000, 1300]]
CARRY_RESET = [0, 0, 1, 0]


def carry_rows():
    """-> (call 1 rows, call 2 rows), each a list of S (x, y, p, t)"""
    first, second = [], []
    for kw, split in zip((_C0, _C1, None, _C3), CARRY_SPLIT):
        if kw is None:
            first.append(stream(**_C2_OLD))
            second.append(stream(**_C2_NEW))
        else:
            cols = stream(**kw)
            first.append(tuple(c[:split] for c in cols))
            second.append(tuple(c[split:] for c in cols))
    return first, second


def _case(rep_mod, rows, fkw, ends, out, key):
    ends = np.asarray(ends, np.int64)                                  # [T, S]
    frames, bounds, t_sha, t_last = [], [], [], []
    for s, (x, y, p, t) in enumerate(rows):
        f, tc, b = reference_frames(rep_mod, x, y, p, t, fkw, ends[:, s])
        frames.append(f)
        bounds.append(b)
        t_sha.append(sha256(tc.astype(np.int64)))
        t_last.append(int(tc.max()) if len(tc) else 0)
    out[f"{key}/frames"] = np.stack(frames, 1)                         # [T, S, C, H', W']
    out[f"{key}/bounds"] = np.stack(bounds, 1).astype(np.int64)        # [T, S, 2], indices into the row
    out[f"{key}/t_sha256"] = np.array(t_sha)
    out[f"{key}/t_last"] = np.array(t_last, np.int64)


def generate() -> dict:
    rep_mod = load_representations()
    out = {}
    rows = [stream(**kw) for kw in ROWS]
    _case(rep_mod, rows, DURATION_KW, DURATION_ENDS, out, "duration")
    _case(rep_mod, rows, COUNT_KW, COUNT_ENDS, out, "count")
    # what call 2 must give: every row the reference on call 2's events from that row's carry (0 for the row that starts a new
    # recording); for the rows that continue and have new events that is the whole recording in one piece, bounds shifted by the split
    first, second = carry_rows()
    ends = np.asarray(CARRY_ENDS, np.int64)
    frames, bounds, t_sha, t_last = [], [], [], []
    for s in range(4):
        carry = 0 if CARRY_RESET[s] else int(correct_time(first[s][3]).max())
        f, tc, b = reference_frames(rep_mod, *second[s], CARRY_KW, ends[:, s], t_carry=carry)
        if not CARRY_RESET[s] and len(tc):
            split = CARRY_SPLIT[s]
            whole = [np.concatenate([u, v]) for u, v in zip(first[s], second[s])]
            f1, tc1, b1 = reference_frames(rep_mod, *whole, CARRY_KW, ends[:, s])
            assert (b1[:, 0] >= split).all(), f"carry case, row {s}: every window must start in call 2's events"
            assert np.array_equal(f1, f) and np.array_equal(b1 - split, b) and np.array_equal(tc1[split:], tc)
        frames.append(f)
        bounds.append(b)
        t_sha.append(sha256(tc.astype(np.int64)))
        t_last.append(max(carry, int(tc.max()) if len(tc) else 0))
    # the carry has work to do: without it (or with another row's) call 2's corrected timestamps differ
    assert not np.array_equal(correct_time(second[0][3]), correct_time(second[0][3], int(correct_time(first[0][3]).max())))
    assert not np.array_equal(correct_time(second[3][3]), correct_time(second[3][3], int(correct_time(first[3][3]).max())))
    out["carry/frames"] = np.stack(frames, 1)
    out["carry/bounds"] = np.stack(bounds, 1).astype(np.int64)
    out["carry/t_sha256"] = np.array(t_sha)
    out["carry/t_last"] = np.array(t_last, np.int64)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
