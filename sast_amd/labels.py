"""Raw Prophesee box labels -> window ends and label tensors on the GPU (csrc/k_labels.hip).

The reference derives both offline, per recording, from the label timestamps: scripts/genx/preprocess_dataset.py:336-428
(`labels_and_ev_repr_timestamps`) filters the boxes (:191-284), accepts the label times that sit on a jittered 4 Hz (gen1) / ~10 Hz (gen4)
grid, and places the event windows by `np.linspace` between accepted label times; `ObjectLabelFactory` (data/genx_utils/labels.py:
149-198) then clamps and, for the downsampled Gen4 input, halves the boxes of a label frame when a sample is read.  `LabelStreams` does
all of it on the device for S recordings side by side and hands out, per step, the tensors the rest of the chain takes:
`ends_us` for `EventStreams` / `EventQueue.frames`, `(labels, counts)` for `SpatialAugmentor.__call__`, the YOLOX loss and
`PropheseeEvaluator.add`.  Integers equal the reference's, fp32 values equal it bit for bit.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _frontend as F
from . import _lib as L
from .functional import _need_gpu, _stream

BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})
DATASET_HW = {'gen1': (240, 304), 'gen4': (720, 1280)}                 # preprocess_dataset.py:54-55
# conf_preprocess/filter_*.yaml: apply_psee_bbox_filter, apply_faulty_bbox_filter
FILTER_DEFAULTS = {'gen1': (True, True), 'gen4': (False, True)}

# status bits of a row, lowest first (include/sast_hip.h, SAST_LABELS_*)
FLAGS = (
    (L.LABELS_UNSORTED, "unsorted", "the records are not sorted by t"),
    (L.LABELS_NEGATIVE_SIZE, "negative_size", "a record has a negative w or h"),
    (L.LABELS_NO_LABELS, "no_labels", "no label survives the filters"),
    (L.LABELS_BAD_RATE, "bad_rate", "the gen4 label rate is not 30 / 60 Hz, or there are fewer than two unique timestamps"),
    (L.LABELS_NO_ALIGNED_LABEL, "no_aligned_label", "no label at or after align_t_ms"),
    (L.LABELS_ZERO_COUNT, "zero_count", "a label timestamp lies within 2 ms of the last label frame"),
    (L.LABELS_TOO_MANY_FRAMES, "too_many_frames", "more than max_frames label frames"),
    (L.LABELS_TOO_MANY_WINDOWS, "too_many_windows", "more than max_windows windows"),
    (L.LABELS_FRAME_OVERFULL, "frame_overfull", "a label frame holds more than max_labels_per_frame boxes; it was cut to the first ones"),
    (L.LABELS_FRAMES_TOO_CLOSE, "frames_too_close", "two label frames are <= 98 000 us apart"),
    (L.LABELS_WINDOW_INDEX, "window_index", "labels() was given a window index outside [0, n_windows)"),
)


def flag_names(status: int) -> Tuple[str, ...]:
    return tuple(name for bit, name, _msg in FLAGS if status & bit)


class _Labels(NamedTuple):
    labels: torch.Tensor
    counts: torch.Tensor
    ends_us: torch.Tensor
    labelled: torch.Tensor


class LabelStreams:
    """ls = LabelStreams(num_streams, capacity, dataset='gen1' | 'gen4', split='train' | 'val' | 'test', ..., max_frames, max_windows,
                        max_labels_per_frame)
    ls.load(records, counts, reset=None, check=False)     once per recording and row
    labels, counts, ends_us, labelled = ls.labels(window_idx, out=None)
    ls.labelled_windows()                                 per row, which windows are label frames (host copy, once after load)

    records: int32 [S, capacity, 10] on the device, row s the 40-byte BBOX_DTYPE records of one recording as ten little-endian words
      (`LabelStreams.pack` makes them from a structured array), sorted by t, the first counts[s] (int64 [S]) of them valid.
    load: rows with reset[s] != 0 (uint8 / bool [S]; default: every row) are rebuilt, the others are left as they are.  Per row, in the
      reference's order: the filters of apply_filters (gen4: class_id <= 2; crop to the frame; Prophesee's size filter -- diagonal 30 /
      side 10 for gen1, 60 / 20 for gen4 -- with apply_psee_bbox_filter, else sides >= 5; for split 'train' with
      apply_faulty_bbox_filter, w <= (9 * W) // 10), the unique timestamps, the base delta (gen1: 250 000; gen4: from np.median of their
      differences), the label frames (the first unique timestamp >= align_t_ms, then every one whose distance to the last label frame
      is within 2 ms of a multiple of the base delta), the window ends (a lead-in in steps of ts_step_ev_repr_ms, then np.linspace
      between label frames), frame_2_window, and the label frames' boxes through ObjectLabelFactory (clamp_to_frame_; with
      downsample_by_2, scale_(0.5) and its removal of flat boxes).
    State after load, all device tensors: ends_us int64 [S, max_windows], n_windows int32 [S], frame_ts_us int64 [S, max_frames],
      n_frames int32 [S], frame_2_window int64 [S, max_frames], window_2_frame int32 [S, max_windows] (-1: not a label frame),
      label_rows fp32 [S, capacity, 7] = (t, x, y, w, h, class_id, class_confidence) in frame order, frame_start / frame_count int32
      [S, max_frames], status int32 [S].
    status: a bit per condition (`FLAGS`; `errors()` names them per row, which synchronises).  A flagged row has n_frames = n_windows =
      0, except for frame_overfull (the frame is cut to its first max_labels_per_frame boxes) and window_index (set by `labels`).
      check=True on load synchronises and raises ValueError naming the first flagged row and its first flag.
    labels(window_idx): int64 [S] or [T, S] on the device -> labels fp32 [T, S, M, 7] (M = max_labels_per_frame; a frame's rows at the
      front, zeros behind: the layout `SpatialAugmentor.__call__` and `PropheseeEvaluator.add` take as [T * S, M, 7]), counts int32
      [T, S], ends_us int64 [T, S], labelled uint8 [T, S].  counts is 0 where the window is no label frame or all its boxes vanished in
      the downscale; labelled tells the two apart.  An index outside [0, n_windows[s]) gives counts 0, ends_us -1, labelled 0 and sets
      window_index in status[s].  out: the four tensors to write.
    Launches: 1 per load, 1 per labels, whatever S, T and the counts are (a 1024-thread workgroup per row; every count is read on the
      device).  After one un-captured call of each method nothing is allocated but `out` and nothing synchronises, so labels +
      EventStreams (or EventQueue.frames) + SpatialAugmentor can be captured in one graph and replayed with new indices written into
      the same tensor."""

    LOAD_LAUNCHES = 1
    LABELS_LAUNCHES = 1

    def __init__(self, num_streams: int, capacity: int, dataset: str = 'gen1', split: str = 'train',
                 apply_psee_bbox_filter: Optional[bool] = None, apply_faulty_bbox_filter: Optional[bool] = None, align_t_ms: int = 100,
                 ts_step_ev_repr_ms: int = 50, downsample_by_2: bool = False, max_frames: int = 4096, max_windows: int = 16384,
                 max_labels_per_frame: int = 64):
        if dataset not in DATASET_HW:
            raise ValueError(f"sast_amd.labels: dataset must be 'gen1' or 'gen4', got {dataset!r}")
        if split not in ('train', 'val', 'test'):
            raise ValueError(f"sast_amd.labels: split must be 'train', 'val' or 'test', got {split!r}")
        ts_step_ev_repr_ms, align_t_ms = int(ts_step_ev_repr_ms), int(align_t_ms)
        if ts_step_ev_repr_ms <= 0 or 100 % ts_step_ev_repr_ms != 0:            # preprocess_dataset.py:344-346
            raise ValueError("sast_amd.labels: ts_step_ev_repr_ms must be > 0 and divide 100")
        if align_t_ms < 0:
            raise ValueError("sast_amd.labels: align_t_ms must be >= 0")
        F.stream_count(num_streams, "labels")
        if int(capacity) < 1 or int(num_streams) * int(capacity) > (2 ** 31 - 1) // 16:
            raise ValueError("sast_amd.labels: capacity must be >= 1 and num_streams * capacity <= (2^31 - 1) / 16")
        for v, name in ((max_frames, "max_frames"), (max_windows, "max_windows"), (max_labels_per_frame, "max_labels_per_frame")):
            if int(v) < 1 or int(num_streams) * int(v) > 2 ** 31 - 1:
                raise ValueError(f"sast_amd.labels: {name} must be >= 1 and num_streams * {name} below 2^31")
        self.num_streams, self.capacity = int(num_streams), int(capacity)
        self.dataset, self.split = dataset, split
        psee, faulty = FILTER_DEFAULTS[dataset]
        self.apply_psee_bbox_filter = psee if apply_psee_bbox_filter is None else bool(apply_psee_bbox_filter)
        self.apply_faulty_bbox_filter = faulty if apply_faulty_bbox_filter is None else bool(apply_faulty_bbox_filter)
        self.align_t_ms, self.ts_step_ev_repr_ms = align_t_ms, ts_step_ev_repr_ms
        self.downsample_by_2 = bool(downsample_by_2)
        self.max_frames, self.max_windows, self.max_labels_per_frame = int(max_frames), int(max_windows), int(max_labels_per_frame)
        self.height, self.width = DATASET_HW[dataset]
        self.ends_us = self.n_windows = self.frame_ts_us = self.n_frames = self.frame_2_window = self.window_2_frame = None
        self.label_rows = self.frame_start = self.frame_count = self.status = None
        self._args = None
        self._ws = None

    @staticmethod
    def pack(boxes: np.ndarray) -> np.ndarray:
        """a structured array with the fields t (or ts), x, y, w, h, class_id, class_confidence (or confidence) and optionally track_id
        -> int32 [n, 10], the BBOX_DTYPE records as words (reformat_boxes, box_loading.py:27-44)"""
        names = boxes.dtype.names or ()
        alias = {'ts': 't', 'confidence': 'class_confidence'}
        have = {alias.get(n, n) for n in names}
        missing = [n for n in ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence') if n not in have]
        if missing:
            raise ValueError(f"sast_amd.labels: the box array lacks the fields {missing}")
        new = np.zeros(boxes.shape[0], dtype=BBOX_DTYPE)
        for n in names:
            if alias.get(n, n) in BBOX_DTYPE.names:
                new[alias.get(n, n)] = boxes[n]
        return new.view(np.int32).reshape(boxes.shape[0], 10)

    def _storage(self, dev):
        """the state on `dev` (allocated by the first ordinary call)"""
        if self._args is not None:
            F.lives_on("the state", self.status.device, "the call's tensors", dev, "labels")
        else:
            F.not_capturing("labels")
            S, cap, Fr, W = self.num_streams, self.capacity, self.max_frames, self.max_windows
            i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
            self.ends_us, self.n_windows = torch.zeros(S, W, **i64), torch.zeros(S, **i32)
            self.frame_ts_us, self.n_frames = torch.zeros(S, Fr, **i64), torch.zeros(S, **i32)
            self.frame_2_window, self.window_2_frame = torch.zeros(S, Fr, **i64), torch.full((S, W), -1, **i32)
            self.label_rows = torch.zeros(S, cap, 7, dtype=torch.float32, device=dev)
            self.frame_start, self.frame_count, self.status = torch.zeros(S, Fr, **i32), torch.zeros(S, Fr, **i32), torch.zeros(S, **i32)
            nbytes = int(L.lib().sast_labels_ws_bytes(S, cap, Fr))
            if nbytes == 0:
                raise ValueError("sast_amd.labels: unsupported sizes")
            self._ws = torch.zeros((nbytes + 7) // 8, **i64)
            a = self._args = L.SastLabelArgs()
            a.ws, a.ends_us, a.n_windows = self._ws.data_ptr(), self.ends_us.data_ptr(), self.n_windows.data_ptr()
            a.frame_ts_us, a.n_frames = self.frame_ts_us.data_ptr(), self.n_frames.data_ptr()
            a.frame_2_window, a.window_2_frame = self.frame_2_window.data_ptr(), self.window_2_frame.data_ptr()
            a.labels, a.frame_start, a.frame_count = self.label_rows.data_ptr(), self.frame_start.data_ptr(), self.frame_count.data_ptr()
            a.status = self.status.data_ptr()
            a.capacity, a.S, a.width, a.height = cap, S, self.width, self.height
            a.base_delta_us = 250000 if self.dataset == 'gen1' else 0             # preprocess_dataset.py:287-299
            a.align_t_us, a.delta_t_us = self.align_t_ms * 1000, self.ts_step_ev_repr_ms * 1000
            a.reprs_per_frame = 100 // self.ts_step_ev_repr_ms
            a.class_max = 2 if self.dataset == 'gen4' else -1
            gen4 = self.dataset == 'gen4'
            if self.apply_psee_bbox_filter:                                     # :191-206
                a.min_diag2, a.min_side = float((60 if gen4 else 30) ** 2), float(20 if gen4 else 10)
            else:                                                               # :209-215
                a.min_diag2, a.min_side = 0.0, 5.0
            faulty = self.split == 'train' and self.apply_faulty_bbox_filter     # :282-283
            a.max_width = float((9 * self.width) // 10) if faulty else -1.0
            a.downsample_by_2 = int(self.downsample_by_2)
            a.max_frames, a.max_windows, a.max_labels_per_frame = Fr, W, self.max_labels_per_frame
        return self._args

    def errors(self) -> List[Tuple[str, ...]]:
        """the names of the flags of every row (synchronises)"""
        if self.status is None:
            return [()] * self.num_streams
        return [flag_names(int(v)) for v in self.status.tolist()]

    def load(self, records: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None, check: bool = False) -> None:
        S, cap = self.num_streams, self.capacity
        F.tensor_arg(records, "records", "labels", (torch.int32,), (S, cap, 10), "(ten words per box record)", dtype_error=TypeError)
        F.counts_reset(counts, reset, S, "labels")
        _need_gpu(records, counts, reset)
        F.same_device("labels", "records, counts and reset", records, counts, reset)
        a = self._storage(records.device)
        L.check(L.lib().sast_labels_load(C.byref(a), records.data_ptr(), counts.data_ptr(), None if reset is None else reset.data_ptr(),
                                         _stream()), "labels_load")
        if check:
            for s, v in enumerate(self.status.tolist()):
                for bit, name, msg in FLAGS:
                    if v & bit:
                        raise ValueError(f"sast_amd.labels: row {s}: {name}: {msg}")

    def labelled_windows(self) -> List[np.ndarray]:
        """per row a numpy bool array over its n_windows windows: True where the window ends at a label frame (window_2_frame >= 0),
        whether or not any of its boxes survives the filters or a later augmentation -- the pairs the training step selects
        (modules/detection.py:161-171).  ONE synchronising copy, meant to be called once after `load`: a loader then knows the number K
        of labelled (timestep, sample) pairs of every step (the batch of the PAFPN / head pass, `functional.SelectionTable`'s n_out)
        without a sync per step."""
        if self._args is None:
            raise RuntimeError("sast_amd.labels: call load() before labelled_windows()")
        both = torch.cat([self.n_windows.view(-1, 1), self.window_2_frame], dim=1).cpu().numpy()
        return [both[s, 1:1 + int(both[s, 0])] >= 0 for s in range(self.num_streams)]

    def labels(self, window_idx: torch.Tensor, out=None):
        S, M = self.num_streams, self.max_labels_per_frame
        T = F.window_ends(window_idx, S, "labels", "window_idx")
        _need_gpu(window_idx)
        if self._args is None:
            raise RuntimeError("sast_amd.labels: call load() before labels()")
        dev = window_idx.device
        F.lives_on("the state", self.status.device, "window_idx", dev, "labels")
        if T * S * M > (2 ** 31 - 1) // 8:
            raise ValueError("sast_amd.labels: T * num_streams * max_labels_per_frame must be <= (2^31 - 1) / 8")
        shape = tuple(window_idx.shape)
        want = ((shape + (M, 7), torch.float32), (shape, torch.int32), (shape, torch.int64), (shape, torch.uint8))
        out = tuple(F.outputs(_Labels, want, out, dev, "labels", "four tensors (labels, counts, ends_us, labelled)", "the state's"))
        L.check(L.lib().sast_labels_gather(C.byref(self._args), window_idx.data_ptr(), T, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), out[3].data_ptr(), _stream()), "labels_gather")
        return out
