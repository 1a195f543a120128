"""Track ids for online detections, on the device (csrc/k_track.hip): a greedy IoU tracker without a motion model.

The reference has no tracker, and its detections leave with `track_id = 0`.  `DetectionTracker` fills that word: one launch per
online step between `online.export_detections` and `DetectionLog.append`, predicated per row by `due` and following `reset`, with no
allocation and no synchronisation -- so it sits inside `OnlineDetector`'s captured push.  The rule (expire by age, greedy matching by
IoU in a strict total order, births into the lowest free slots) is written out in include/sast_hip.h and stated sequentially in
tests/tracker_model.py.  It is this project's own: parity with any external tracker is not claimed.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _frontend as F
from . import _lib as L
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
