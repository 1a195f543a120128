"""Track ids for online detections, on the device (csrc/k_track.hip): a greedy IoU tracker without a motion model.

The reference has no tracker, and its detections leave with `track_id = 0`.  `DetectionTracker` fills that word: one launch per
online step between `online.export_detections` and `DetectionLog.append`, predicated per row by `due` and following `reset`, with no
allocation and no synchronisation -- so it sits inside `OnlineDetector`'s captured push.  The rule (expire by age, greedy matching by
IoU in a strict total order, births into the lowest free slots) is written out in include/sast_hip.h and stated sequentially in
tests/tracker_model.py.  It is this project's own: parity with any external tracker is not claimed.

`TrackingEvaluator` (csrc/k_trackeval.hip) reads the ids back: the CLEAR-MOT counts of tracked detections against the labelled tracks
of whole recordings -- matches, misses, false positives, identity switches, fragmentations and the mostly tracked / partially tracked
/ mostly lost tracks, with MOTA, MOTP, recall and precision derived on the host.  It takes the tensors of
`PropheseeEvaluator.add_recordings`, so `DetectionLog.records` or what `track_recordings` filled go in as they are.  Its rule is written
out in include/sast_hip.h ("tracking metrics") and stated sequentially in tests/tracking_eval_model.py.  Parity with py-motmetrics and
TrackEval is not pinned by a test: neither is installed where this project is built.  IDF1 and HOTA need a global assignment over whole
recordings and are not computed.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _frontend as F
from . import _lib as L
from .evaluation import PropheseeEvaluator
from .functional import _need_gpu, _stream

RECORD_BYTES = L.DET_RECORD_BYTES
MAX_TRACKS, MAX_DET, MAX_PAIRS = L.TRACK_MAX_TRACKS, L.TRACK_MAX_DET, L.TRACK_MAX_PAIRS


class DetectionTracker:
    """tr = DetectionTracker(num_streams, max_det, max_tracks=64, iou_thre=0.3, max_age_us=200_000, new_score_thre=0.0, class_agnostic=False)
      max_tracks slots per stream (1 .. 128); a detection continues the live track of its class (any class with class_agnostic) whose
      box it overlaps best, IoU >= iou_thre (in (0, 1]); a track that no detection continued for more than max_age_us is dropped; an
      unmatched detection with class_confidence >= new_score_thre starts a track with the row's next id (1, 2, ...), while a slot is free.
      max_det <= 1792 and max_tracks * max_det <= 65536 (the kernel's LDS plan and the pairs one round sweeps).
    State, allocated by the first, un-captured call and never moved: ids int32 [S, T] (0: free), box fp32 [S, T, 4] (x, y, w, h),
      cls int32 [S, T], last_t int64 [S, T], hits int32 [S, T] (how often the track was seen: a caller's confirmation delay reads it),
      next_id int32 [S], counters int32 [4].
    tr.step(records, counts, ends, due, reset=None): sast_tracker_step on what `export_detections` wrote -- records uint8 [S, max_det', 40]
      with max_det' <= max_det, counts int32 [S], ends int64 [S], due uint8 / bool [S], reset uint8 / bool [S]: the track_id of the first
      counts[s] records of every due row is written, nothing else of a record.  One launch, no synchronisation.
    tr.track_recordings(records, n): sast_tracker_run on whole recordings -- records int32 [S, Dcap, 10] (`DetectionLog.records`, the `dt`
      of `PropheseeEvaluator.add_recordings`), n int64 [S], sorted by t: every row starts from an empty table, every maximal run of
      equal t is one step.  One launch.
    tr.clear(streams=None): from the host, the rows `streams` (default: all, and the counters) start over.
    tr.errors() -> (detections that found no free slot, runs cut by max_det, unsorted rows) (synchronises)."""

    def __init__(self, num_streams: int, max_det: int, max_tracks: int = 64, iou_thre: float = 0.3, max_age_us: int = 200_000,
                 new_score_thre: float = 0.0, class_agnostic: bool = False):
        self.num_streams = F.stream_count(num_streams, "tracking")
        self.max_det, self.max_tracks = int(max_det), int(max_tracks)
        if not 1 <= self.max_tracks <= MAX_TRACKS:
            raise ValueError(f"sast_amd.tracking: max_tracks must be in 1 .. {MAX_TRACKS}, got {max_tracks}")
        if not 1 <= self.max_det <= MAX_DET or self.max_tracks * self.max_det > MAX_PAIRS:
            raise ValueError(f"sast_amd.tracking: max_det must be in 1 .. {MAX_DET} and max_tracks * max_det <= {MAX_PAIRS}, got "
                             f"max_det {max_det} with max_tracks {max_tracks}")
        self.iou_thre, self.new_score_thre = float(iou_thre), float(new_score_thre)
        if not 0.0 < self.iou_thre <= 1.0:
            raise ValueError(f"sast_amd.tracking: iou_thre must be in (0, 1], got {iou_thre}")
        if math.isnan(self.new_score_thre):
            raise ValueError("sast_amd.tracking: new_score_thre must not be NaN")
        self.max_age_us = int(max_age_us)
        if self.max_age_us < 0:
            raise ValueError(f"sast_amd.tracking: max_age_us must be >= 0, got {max_age_us}")
        self.class_agnostic = bool(class_agnostic)
        self.ids = self.box = self.cls = self.last_t = self.hits = self.next_id = self.counters = None

    def _args(self, dev: torch.device, max_det: int):
        if self.ids is None:
            F.not_capturing("tracking", "one un-captured call is needed before graph capture (it allocates the track tables)")
            S, T = self.num_streams, self.max_tracks
            self.ids = torch.zeros(S, T, dtype=torch.int32, device=dev)
            self.box = torch.zeros(S, T, 4, dtype=torch.float32, device=dev)
            self.cls = torch.zeros(S, T, dtype=torch.int32, device=dev)
            self.last_t = torch.zeros(S, T, dtype=torch.int64, device=dev)
            self.hits = torch.zeros(S, T, dtype=torch.int32, device=dev)
            self.next_id = torch.ones(S, dtype=torch.int32, device=dev)
            self.counters = torch.zeros(4, dtype=torch.int32, device=dev)
        else:
            F.lives_on("the tracker", self.ids.device, "the records", dev, "tracking")
        a = L.SastTrackerArgs()
        a.ids, a.box, a.cls, a.last_t, a.hits = (self.ids.data_ptr(), self.box.data_ptr(), self.cls.data_ptr(), self.last_t.data_ptr(),
                                                 self.hits.data_ptr())
        a.next_id, a.counters = self.next_id.data_ptr(), self.counters.data_ptr()
        a.S, a.max_tracks, a.max_det, a.class_agnostic = self.num_streams, self.max_tracks, max_det, int(self.class_agnostic)
        a.iou_thre, a.new_score_thre, a.max_age_us = self.iou_thre, self.new_score_thre, self.max_age_us
        return a

    def step(self, records: torch.Tensor, counts: torch.Tensor, ends: torch.Tensor, due: torch.Tensor,
             reset: Optional[torch.Tensor] = None) -> None:
        S = self.num_streams
        F.tensor_arg(records, "records", "tracking", (torch.uint8,), (("num_streams", S), "max_det", RECORD_BYTES))
        if records.shape[1] > self.max_det:
            raise ValueError(f"sast_amd.tracking: records hold {records.shape[1]} per row, the tracker was made for max_det {self.max_det}")
        F.tensor_arg(counts, "counts", "tracking", (torch.int32,), (S,))
        F.tensor_arg(ends, "ends", "tracking", (torch.int64,), (S,))
        F.flags(due, "due", S, "tracking")
        if due is None:
            raise ValueError("sast_amd.tracking: due must be a uint8 / bool tensor of shape [num_streams]")
        F.flags(reset, "reset", S, "tracking")
        _need_gpu(records, counts, ends, due, reset)
        F.same_device("tracking", "records, counts, ends, due and reset", records, counts, ends, due, reset)
        a = self._args(records.device, records.shape[1])
        st = L.SastTrackStepArgs()
        st.records, st.counts, st.ends, st.due = records.data_ptr(), counts.data_ptr(), ends.data_ptr(), due.data_ptr()
        st.reset = None if reset is None else reset.data_ptr()
        L.check(L.lib().sast_tracker_step(C.byref(a), C.byref(st), _stream()), "tracker_step")

    def track_recordings(self, records: torch.Tensor, n: torch.Tensor) -> None:
        S = self.num_streams
        F.tensor_arg(records, "records", "tracking", (torch.int32,), (("num_streams", S), "Dcap", RECORD_BYTES // 4))
        F.tensor_arg(n, "n", "tracking", (torch.int64,), (S,))
        if S * records.shape[1] > (1 << 31) - 1:
            raise ValueError("sast_amd.tracking: num_streams * Dcap must be <= 2^31 - 1")
        _need_gpu(records, n)
        F.same_device("tracking", "records and n", records, n)
        a = self._args(records.device, self.max_det)
        ru = L.SastTrackRunArgs()
        ru.records, ru.n, ru.Dcap = records.data_ptr(), n.data_ptr(), records.shape[1]
        L.check(L.lib().sast_tracker_run(C.byref(a), C.byref(ru), _stream()), "tracker_run")

    def clear(self, streams=None) -> None:
        """a free slot is zero in every table, so clearing is zeroing; the ids then start at 1 again"""
        if self.ids is None:
            return
        F.reset_rows((self.ids, self.box, self.cls, self.last_t, self.hits, self.next_id), self.counters, streams, self.num_streams, "tracking")
        self.next_id += (self.next_id == 0).to(torch.int32)

    def errors(self) -> Tuple[int, int, int]:
        return F.counters(self.counters, 4)[:3]


COUNT_KEYS = ("frames", "gt", "hyp", "matches", "fp", "fn", "idsw", "frag", "gt_tracks", "mt", "pt", "ml")     # the columns SAST_TE_FRAMES ..
ERROR_KEYS = ("unsorted", "refused_labels", "refused_hyp", "refused_tracks", "untracked", "bad_class", "duplicate_labels", "duplicate_hyp")
MAX_FRAME, MAX_GT_TRACKS = L.TRACKEVAL_MAX_FRAME, L.TRACKEVAL_MAX_GT_TRACKS
assert len(COUNT_KEYS) == L.TRACKEVAL_COLS and len(ERROR_KEYS) == L.TRACKEVAL_DIAG and MAX_FRAME == MAX_TRACKS


def _ratio(num: float, den: float) -> float:
    return float(num) / float(den) if den else math.nan


class TrackingEvaluator:
    """te = TrackingEvaluator(dataset, downsample_by_2, iou_thre=0.5, time_tol_us=0, class_agnostic=False, max_gt_tracks=1024,
                           max_labels_per_frame=64, max_hyp_per_frame=128)
      dataset, downsample_by_2: `PropheseeEvaluator`'s -- its classes and its box filter.  A label and a hypothesis may pair when their
      classes are equal (any classes with class_agnostic) and their IoU, the tracker's fp32 one, is >= iou_thre (in (0, 1]); a frame is
      a unique label timestamp, its hypotheses the detection run nearest in time within time_tol_us (>= 0; the earlier run on a tie).
      max_labels_per_frame, max_hyp_per_frame in 1 .. 128 and max_gt_tracks (distinct label ids of a recording) in 1 .. 65536: a
      recording past one of them is refused whole.
    te.add_recordings(gt, n_gt, dt, n_dt): the tensors of `PropheseeEvaluator.add_recordings` -- label records int32 [S, Gcap, 10] /
      int64 [S] against detection records int32 [S, Dcap, 10] / int64 [S], both sorted by t; word 7, track_id, is the ground-truth track
      of a label and the tracker's id of a detection (0: untracked, dropped).  Two launches, no synchronisation; after one eager call
      (it allocates the track tables and the rows) it is capturable, and a replay scores the records then in the same tensors.
    te.rows -> (int64 [S, K + 1, 12], fp64 [S, K + 1]): the counts (COUNT_KEYS) and the IoU sum of the LAST call per recording and class,
      row K all classes together.
    te.evaluate() -> dict of COUNT_KEYS as ints and MOTA, MOTP, recall, precision as floats (NaN where the denominator is 0), over
      everything added since the last reset.  One synchronisation.  Raises ValueError when a recording was not sorted by t and
      OverflowError when one was refused for a limit: those recordings added nothing.
    te.per_class() -> {class name: such a dict}; te.merge(other) adds another evaluator's accumulator; te.reset() clears this one's;
    te.errors() -> dict of ERROR_KEYS (synchronises): the recordings refused, and the records dropped as untracked (track_id 0), for a
      class id past the dataset's, or as a second record of their track_id in a frame."""

    def __init__(self, dataset: str, downsample_by_2: bool, iou_thre: float = 0.5, time_tol_us: int = 0, class_agnostic: bool = False,
                 max_gt_tracks: int = 1024, max_labels_per_frame: int = 64, max_hyp_per_frame: int = 128):
        task = PropheseeEvaluator(dataset, downsample_by_2)            # the classes and the filter thresholds are the evaluator's
        self.dataset, self.downsample_by_2, self.classes = task.dataset, task.downsample_by_2, task.classes
        self.min_box_diag, self.min_box_side = task.min_box_diag, task.min_box_side
        self.iou_thre, self.time_tol_us, self.class_agnostic = float(iou_thre), int(time_tol_us), bool(class_agnostic)
        self.max_gt_tracks, self.max_labels_per_frame, self.max_hyp_per_frame = int(max_gt_tracks), int(max_labels_per_frame), int(max_hyp_per_frame)
        if not 0.0 < self.iou_thre <= 1.0:
            raise ValueError(f"sast_amd.tracking: iou_thre must be in (0, 1], got {iou_thre}")
        if self.time_tol_us < 0:
            raise ValueError(f"sast_amd.tracking: time_tol_us must be >= 0, got {time_tol_us}")
        if not 1 <= self.max_labels_per_frame <= MAX_FRAME or not 1 <= self.max_hyp_per_frame <= MAX_FRAME:
            raise ValueError(f"sast_amd.tracking: max_labels_per_frame and max_hyp_per_frame must be in 1 .. {MAX_FRAME}, got "
                             f"{max_labels_per_frame} and {max_hyp_per_frame}")
        if not 1 <= self.max_gt_tracks <= MAX_GT_TRACKS:
            raise ValueError(f"sast_amd.tracking: max_gt_tracks must be in 1 .. {MAX_GT_TRACKS}, got {max_gt_tracks}")
        self._acc = self._rows = self._rows_iou = self._rows_diag = self._ws = None
        self._last_S, self._retired = 0, []                    # buffers a call with more recordings replaced: a captured graph may hold them
        self._args = L.SastTrackEvalArgs()

    # the accumulator is ONE int64 tensor, so that evaluate() copies once: [K + 1, 12] counts, K + 1 fp64 IoU sums (as bits), 8 error words
    def _views(self, acc: torch.Tensor):
        K1, NC = len(self.classes) + 1, L.TRACKEVAL_COLS
        return acc[:K1 * NC].view(K1, NC), acc[K1 * NC:K1 * NC + K1].view(torch.float64), acc[K1 * NC + K1:]

    def _new_accumulator(self, dev: torch.device) -> None:
        a = self._args
        self._acc = torch.zeros((len(self.classes) + 1) * (L.TRACKEVAL_COLS + 1) + L.TRACKEVAL_DIAG, dtype=torch.int64, device=dev)
        counts, iou, diag = self._views(self._acc)
        a.acc, a.acc_iou, a.acc_diag = counts.data_ptr(), iou.data_ptr(), diag.data_ptr()
        a.K, a.class_agnostic = len(self.classes), int(self.class_agnostic)
        a.max_gt_tracks, a.max_labels_per_frame, a.max_hyp_per_frame = self.max_gt_tracks, self.max_labels_per_frame, self.max_hyp_per_frame
        a.iou_thre, a.time_tol_us = self.iou_thre, self.time_tol_us
        a.min_diag2, a.min_side = float(self.min_box_diag ** 2), float(self.min_box_side)

    def _allocate(self, dev: torch.device, S: int) -> None:
        F.not_capturing("tracking", "one un-captured call is needed before graph capture (it allocates the track tables and the rows)")
        K1, NC, ND = len(self.classes) + 1, L.TRACKEVAL_COLS, L.TRACKEVAL_DIAG
        a = self._args
        if self._acc is None:
            self._new_accumulator(dev)
        a.ws_bytes = int(L.lib().sast_trackeval_ws_bytes(S, self.max_gt_tracks))
        if a.ws_bytes == 0:
            raise RuntimeError("sast_amd.tracking: the library refused the track table size")
        self._retired.append((self._ws, self._rows, self._rows_iou, self._rows_diag))
        self._ws = torch.empty(a.ws_bytes, dtype=torch.uint8, device=dev)
        self._rows = torch.zeros(S, K1, NC, dtype=torch.int64, device=dev)
        self._rows_iou = torch.zeros(S, K1, dtype=torch.float64, device=dev)
        self._rows_diag = torch.zeros(S, ND, dtype=torch.int64, device=dev)
        a.ws, a.rows, a.rows_iou, a.rows_diag = self._ws.data_ptr(), self._rows.data_ptr(), self._rows_iou.data_ptr(), self._rows_diag.data_ptr()

    def add_recordings(self, gt: torch.Tensor, n_gt: torch.Tensor, dt: torch.Tensor, n_dt: torch.Tensor) -> None:
        F.tensor_arg(gt, "gt", "tracking", (torch.int32,), ("S", "Gcap", RECORD_BYTES // 4), "(ten words per box record)", dtype_error=TypeError)
        S, Gcap = int(gt.shape[0]), int(gt.shape[1])
        F.tensor_arg(n_gt, "n_gt", "tracking", (torch.int64,), (S,), dtype_error=TypeError)
        F.tensor_arg(dt, "dt", "tracking", (torch.int32,), (("S", S), "Dcap", RECORD_BYTES // 4), "(ten words per box record)", dtype_error=TypeError)
        Dcap = int(dt.shape[1])
        F.tensor_arg(n_dt, "n_dt", "tracking", (torch.int64,), (S,), dtype_error=TypeError)
        if S > 65535 or S * max(Gcap, Dcap) > (1 << 31) - 257:
            raise ValueError("sast_amd.tracking: need S <= 65535 recordings and S * Gcap, S * Dcap <= 2^31 - 257 records")
        _need_gpu(gt, n_gt, dt, n_dt)
        F.same_device("tracking", "gt, n_gt, dt and n_dt", gt, n_gt, dt, n_dt)
        if self._acc is not None:
            F.lives_on("the evaluator", self._acc.device, "the records", gt.device, "tracking")
        if self._rows is None or self._rows.shape[0] < S:        # sized by the largest S so far; fewer recordings use the front
            self._allocate(gt.device, S)
        self._last_S = S
        a = self._args
        a.gt, a.n_gt, a.dt, a.n_dt = gt.data_ptr(), n_gt.data_ptr(), dt.data_ptr(), n_dt.data_ptr()
        a.S, a.Gcap, a.Dcap = S, Gcap, Dcap
        L.check(L.lib().sast_trackeval_add(C.byref(a), _stream()), "trackeval_add")

    @property
    def rows(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._rows is None:
            raise RuntimeError("sast_amd.tracking: rows follow an add_recordings")
        return self._rows[:self._last_S], self._rows_iou[:self._last_S]

    def reset(self) -> None:
        """the accumulator and the error words back to zero: one launch, no synchronisation"""
        if self._acc is not None:
            L.check(L.lib().sast_trackeval_reset(C.byref(self._args), _stream()), "trackeval_reset")

    def merge(self, other: "TrackingEvaluator") -> None:
        """other's accumulator added to this one's, as if its recordings had been added here (the IoU sums: this one's plus other's)"""
        if not isinstance(other, TrackingEvaluator):
            raise TypeError("sast_amd.tracking: merge takes another TrackingEvaluator")
        mine = (self.dataset, self.downsample_by_2, self.iou_thre, self.time_tol_us, self.class_agnostic)
        if mine != (other.dataset, other.downsample_by_2, other.iou_thre, other.time_tol_us, other.class_agnostic):
            raise ValueError("sast_amd.tracking: merge needs evaluators of the same dataset, downsample_by_2, iou_thre, time_tol_us and class_agnostic")
        if other._acc is None:
            return
        if self._acc is None:
            F.not_capturing("tracking", "one un-captured call is needed before graph capture (it allocates the accumulator)")
            self._new_accumulator(other._acc.device)
        F.lives_on("the evaluator", self._acc.device, "the other one", other._acc.device, "tracking")
        for dst, src in zip(self._views(self._acc), other._views(other._acc)):
            dst += src

    def _numbers(self):
        """(counts int64 [K + 1, 12], IoU sums fp64 [K + 1], error words int64 [8]) on the host: the one synchronisation"""
        K1, NC = len(self.classes) + 1, L.TRACKEVAL_COLS
        if self._acc is None:
            return np.zeros((K1, NC), np.int64), np.zeros(K1, np.float64), np.zeros(L.TRACKEVAL_DIAG, np.int64)
        host = self._acc.cpu().numpy()
        return host[:K1 * NC].reshape(K1, NC), host[K1 * NC:K1 * NC + K1].view(np.float64), host[K1 * NC + K1:]

    @staticmethod
    def _metrics(counts, sum_iou: float) -> Dict[str, float]:
        out = {k: int(v) for k, v in zip(COUNT_KEYS, counts)}
        out["MOTA"] = 1.0 - _ratio(out["fn"] + out["fp"] + out["idsw"], out["gt"])
        out["MOTP"] = _ratio(sum_iou, out["matches"])
        out["recall"] = _ratio(out["matches"], out["gt"])
        out["precision"] = _ratio(out["matches"], out["matches"] + out["fp"])
        return out

    def _checked(self):
        counts, iou, diag = self._numbers()
        if diag[L.TE_UNSORTED]:
            raise ValueError(f"sast_amd.tracking: {int(diag[L.TE_UNSORTED])} recording(s) given to add_recordings were not sorted by t (labels "
                             "or detections) and were not evaluated")
        refused = {"max_labels_per_frame": int(diag[L.TE_REFUSED_LABELS]), "max_hyp_per_frame": int(diag[L.TE_REFUSED_HYP]),
                   "max_gt_tracks": int(diag[L.TE_REFUSED_TRACKS])}
        if any(refused.values()):
            raise OverflowError("sast_amd.tracking: recordings did not fit the limits and were not evaluated -- "
                                + ", ".join(f"{v} recording(s) refused for {k}={getattr(self, k)}" for k, v in refused.items() if v))
        return counts, iou

    def evaluate(self) -> Dict[str, float]:
        counts, iou = self._checked()
        return self._metrics(counts[-1], float(iou[-1]))

    def per_class(self) -> Dict[str, Dict[str, float]]:
        counts, iou = self._checked()
        return {name: self._metrics(counts[k], float(iou[k])) for k, name in enumerate(self.classes)}

    def errors(self) -> Dict[str, int]:
        return {k: int(v) for k, v in zip(ERROR_KEYS, self._numbers()[2])}
