"""A numpy model of sast_amd.labels.LabelStreams, one row at a time: the box filters, the label-frame walk, the window-end schedule and
the label tensors of scripts/genx/preprocess_dataset.py:191-428 and data/genx_utils/labels.py:37-50, 149-198, 316-334, restated with
numpy's own fp32 / fp64 operations, plus the status flags and capacities the device class adds.  The CPU tests pin it to the fixture
the reference's functions wrote (tests/golden/label_streams.npz); the GPU tests use it at shapes the fixture does not hold."""
from __future__ import annotations

import numpy as np

BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})
HW = {'gen1': (240, 304), 'gen4': (720, 1280)}
FILTER_DEFAULTS = {'gen1': (True, True), 'gen4': (False, True)}     # apply_psee_bbox_filter, apply_faulty_bbox_filter

# status bits (sast_amd.labels, include/sast_hip.h)
UNSORTED, NEGATIVE_SIZE, NO_LABELS, BAD_RATE, NO_ALIGNED_LABEL, ZERO_COUNT = 1, 2, 4, 8, 16, 32
TOO_MANY_FRAMES, TOO_MANY_WINDOWS, FRAME_OVERFULL, FRAMES_TOO_CLOSE, WINDOW_INDEX = 64, 128, 256, 512, 1024
NOT_FATAL = FRAME_OVERFULL | WINDOW_INDEX


def pack(boxes: np.ndarray) -> np.ndarray:
    """structured boxes -> int32 [n, 10] words of BBOX_DTYPE records ('ts' / 'confidence' spellings accepted)"""
    new = np.zeros(len(boxes), dtype=BBOX_DTYPE)
    for name in boxes.dtype.names:
        new[{'ts': 't', 'confidence': 'class_confidence'}.get(name, name)] = boxes[name]
    return new.view(np.int32).reshape(len(boxes), 10)


def unpack(words: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(words, dtype=np.int32).reshape(-1).view(BBOX_DTYPE)


def apply_filters(b: np.ndarray, dataset: str, split: str, psee: bool, faulty: bool) -> np.ndarray:
    """preprocess_dataset.py:191-284 on a copy of `b`"""
    H, W = HW[dataset]
    b = b.copy()
    if dataset == 'gen4':
        b = b[b['class_id'] <= 2]
    xr, yb = b['x'] + b['w'], b['y'] + b['h']
    xl, yt = np.clip(b['x'], 0, W - 1), np.clip(b['y'], 0, H - 1)
    xr, yb = np.clip(xr, 0, W - 1), np.clip(yb, 0, H - 1)
    b['x'], b['y'], b['w'], b['h'] = xl, yt, xr - xl, yb - yt
    b = b[(b['w'] > 0) & (b['h'] > 0)]
    if psee:
        diag, side = (60, 20) if dataset == 'gen4' else (30, 10)
        b = b[(b['w'] * b['w'] + b['h'] * b['h'] >= np.float32(diag * diag)) & (b['w'] >= side) & (b['h'] >= side)]
    else:
        b = b[(b['w'] >= 5) & (b['h'] >= 5)]
    if split == 'train' and faulty:
        b = b[b['w'] <= (9 * W) // 10]
    return b


class Row:
    """the state of one row after `load`"""

    def __init__(self):
        self.status = 0
        self.ends_us = np.zeros(0, np.int64)
        self.frame_ts_us = np.zeros(0, np.int64)
        self.frame_2_window = np.zeros(0, np.int64)
        self.window_2_frame = np.zeros(0, np.int32)
        self.labels = np.zeros((0, 7), np.float32)
        self.frame_start = np.zeros(0, np.int32)
        self.frame_count = np.zeros(0, np.int32)

    @property
    def n_frames(self):
        return len(self.frame_ts_us)

    @property
    def n_windows(self):
        return len(self.ends_us)


def factory_labels(b: np.ndarray, dataset: str, downsample_by_2: bool) -> np.ndarray:
    """labels.py:166-198 for the boxes of one frame -> fp32 [n, 7]"""
    H, W = HW[dataset]
    L = np.stack([b[k].astype(np.float32) for k in ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')], 1).reshape(-1, 7)
    f = np.float32
    x0, y0 = np.clip(L[:, 1], f(0), f(W - 1)), np.clip(L[:, 2], f(0), f(H - 1))
    x1, y1 = np.clip(L[:, 1] + L[:, 3], f(0), f(W - 1)), np.clip(L[:, 2] + L[:, 4], f(0), f(H - 1))
    L[:, 1], L[:, 2], L[:, 3], L[:, 4] = x0, y0, x1 - x0, y1 - y0
    if downsample_by_2:
        m = f(0.5)
        x1, y1 = np.minimum((L[:, 1] + L[:, 3]) * m, f(0.5 * W - 1)), np.minimum((L[:, 2] + L[:, 4]) * m, f(0.5 * H - 1))
        L[:, 1], L[:, 2] = L[:, 1] * m, L[:, 2] * m
        L[:, 3], L[:, 4] = x1 - L[:, 1], y1 - L[:, 2]
        L = L[(L[:, 3] > 0) & (L[:, 4] > 0)]
    return L


def load_row(words: np.ndarray, dataset: str, split: str, psee=None, faulty=None, align_t_ms=100, ts_step_ev_repr_ms=50,
             downsample_by_2=False, max_frames=1 << 30, max_windows=1 << 30, max_labels_per_frame=1 << 30) -> Row:
    assert 100 % ts_step_ev_repr_ms == 0 and ts_step_ev_repr_ms > 0
    psee = FILTER_DEFAULTS[dataset][0] if psee is None else psee
    faulty = FILTER_DEFAULTS[dataset][1] if faulty is None else faulty
    r = Row()
    b = unpack(words)
    if np.any(np.diff(b['t']) < 0):
        r.status |= UNSORTED
    if np.any(b['w'] < 0) or np.any(b['h'] < 0):
        r.status |= NEGATIVE_SIZE
    if r.status:
        return r
    b = apply_filters(b, dataset, split, psee, faulty)
    if len(b) == 0:
        r.status |= NO_LABELS
        return r
    uts, ustart = np.unique(b['t'].astype(np.int64), return_index=True)
    if dataset == 'gen1':
        base = 250000
    else:
        if len(uts) < 2:
            r.status |= BAD_RATE
            return r
        median = np.median(np.diff(uts))
        hz = int(np.rint(10 ** 6 / median))
        if hz not in (30, 60):
            r.status |= BAD_RATE
            return r
        base = int(6 * median if hz == 60 else 3 * median)
    align_us, delta_us, per_frame = align_t_ms * 1000, ts_step_ev_repr_ms * 1000, 100 // ts_step_ev_repr_ms
    first = int(np.searchsorted(uts, align_us, 'left'))
    if first == len(uts):
        r.status |= NO_ALIGNED_LABEL
        return r
    f0 = int(uts[first])
    lead = max(-(-f0 // delta_us) - 2, 0) if f0 > 0 else 0
    total = lead
    if total + 1 > max_windows:
        r.status |= TOO_MANY_WINDOWS
        return r
    frames, fidx, pair_n = [f0], [first], []
    for j in range(first + 1, len(uts)):
        diff = int(uts[j]) - frames[-1]
        count = int(np.rint(np.float64(diff) / np.float64(base)))
        if abs(diff - count * base) <= 2000:
            if count <= 0:
                r.status |= ZERO_COUNT
            elif len(frames) >= max_frames:
                r.status |= TOO_MANY_FRAMES
            elif diff <= 98000:
                r.status |= FRAMES_TOO_CLOSE
            elif total + count * per_frame + 1 > max_windows:
                r.status |= TOO_MANY_WINDOWS
            if r.status:
                return r
            total += count * per_frame
            pair_n.append(count * per_frame)
            frames.append(int(uts[j]))
            fidx.append(j)
    ends = [f0 - k * delta_us for k in range(lead, 0, -1)]
    for p, n in enumerate(pair_n):
        e = np.linspace(frames[p], frames[p + 1], n + 1).astype(np.int64).tolist()
        ends.extend(e if p == len(pair_n) - 1 else e[:-1])
    if len(frames) == 1:
        ends.append(f0)
    r.ends_us = np.asarray(ends, np.int64)
    assert len(r.ends_us) == total + 1
    r.frame_ts_us = np.asarray(frames, np.int64)
    r.frame_2_window = np.searchsorted(r.ends_us, r.frame_ts_us, 'left').astype(np.int64)
    r.window_2_frame = np.full(len(ends), -1, np.int32)
    r.window_2_frame[r.frame_2_window] = np.arange(len(frames), dtype=np.int32)
    bounds = np.append(ustart, len(b))
    per = []
    for j in fidx:
        L = factory_labels(b[bounds[j]:bounds[j + 1]], dataset, downsample_by_2)
        if len(L) > max_labels_per_frame:
            r.status |= FRAME_OVERFULL
            L = L[:max_labels_per_frame]
        per.append(L)
    r.frame_count = np.asarray([len(L) for L in per], np.int32)
    r.frame_start = (np.cumsum(r.frame_count) - r.frame_count).astype(np.int32)
    r.labels = np.concatenate(per).astype(np.float32).reshape(-1, 7)
    return r


def gather(rows, window_idx: np.ndarray, M: int):
    """LabelStreams.labels on model rows: window_idx int64 [T, S] -> labels [T, S, M, 7], counts, ends_us, labelled (+ flags the rows)"""
    T, S = window_idx.shape
    labels = np.zeros((T, S, M, 7), np.float32)
    counts = np.zeros((T, S), np.int32)
    ends = np.full((T, S), -1, np.int64)
    labelled = np.zeros((T, S), np.uint8)
    for k in range(T):
        for s, r in enumerate(rows):
            w = int(window_idx[k, s])
            if not 0 <= w < r.n_windows:
                r.status |= WINDOW_INDEX
                continue
            ends[k, s] = r.ends_us[w]
            f = int(r.window_2_frame[w])
            if f >= 0:
                n, o = int(r.frame_count[f]), int(r.frame_start[f])
                labelled[k, s], counts[k, s] = 1, n
                labels[k, s, :n] = r.labels[o:o + n]
    return labels, counts, ends, labelled

