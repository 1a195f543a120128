"""Online detection: event chunks in, Prophesee box records out, with no host in the loop (csrc/k_events.hip, k_rows.hip, k_eval.hip).

The reference evaluates recordings offline: frames are built ahead of time (scripts/genx/preprocess_dataset.py), the detector runs
over a dataloader, and detections reach the host through to_prophesee (utils/evaluation/prophesee/io/box_loading.py:58-99).  It has no
stage that follows a live sensor.  `OnlineDetector` is that stage: `EventQueue` retains the events, a scheduler kernel decides on the
device which of each stream's next windows are due, the detector runs a FIXED number of steps per push, and rows whose window is not due
keep their recurrent state -- so S cameras whose windows fall due at different moments share one batch, and the whole push is one
sequence of launches that does not depend on the data: it can be captured in a graph.

The records can leave with track ids: with `tracker=` a `tracking.DetectionTracker` (csrc/k_track.hip: a greedy IoU tracker, this
project's own rule -- the reference has none) every step runs one more launch between the record export and the log, which writes the
`track_id` word of the exported records in place; the log, the pinned slots and `poll()` then carry the ids.  Without one every byte is
what it was: `track_id = 0`.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _frontend as F
from . import _lib as L
from . import functional as SF
from .events import EventQueue
from .functional import _need_gpu, _stream
from .labels import BBOX_DTYPE
from .tracking import DetectionTracker

RECORD_BYTES = L.DET_RECORD_BYTES
assert BBOX_DTYPE.itemsize == RECORD_BYTES


def schedule_windows(queue: EventQueue, next_end: torch.Tensor, first_end_us: int, ends: torch.Tensor, due: torch.Tensor,
                     backlog: torch.Tensor, reset: Optional[torch.Tensor] = None, final: Optional[torch.Tensor] = None) -> None:
    """sast_evq_schedule on the queue's carry: which of each row's next W = ends.shape[0] duration windows are due (an event later than
    the window's end was pushed; with final[s] != 0, also every window that still holds an event time).  next_end int64 [S] is the
    caller's state (first_end_us at the start of a recording; reset[s] != 0 puts it back there first); ends int64 [W, S], due uint8
    [W, S] and backlog int64 [S] are written, next_end advances by the due windows given.  Steps behind a row's due windows repeat the
    last end the row gave (next_end - D when it never gave one), which `queue.frames(ends)` answers without retiring anything new.
    One launch, no synchronisation; call it after `queue.push` on the same stream."""
    S = queue.num_streams
    if queue.mode != L.EVENT_WINDOW_DURATION or queue.value < 1:
        raise ValueError("sast_amd.online: the window schedule needs a queue with duration windows (duration_us >= 1)")
    if int(first_end_us) < queue.value:
        raise ValueError(f"sast_amd.online: first_end_us must be >= duration_us ({queue.value}), got {first_end_us}")
    F.tensor_arg(ends, "ends", "online", (torch.int64,), ("W", S))
    W = ends.shape[0]
    F.tensor_arg(due, "due", "online", (torch.uint8,), (W, S))
    F.tensor_arg(next_end, "next_end", "online", (torch.int64,), (S,))
    F.tensor_arg(backlog, "backlog", "online", (torch.int64,), (S,))
    F.flags(reset, "reset", S, "online")
    F.flags(final, "final", S, "online")
    _need_gpu(next_end, ends, due, backlog, reset, final)
    a = queue._storage(next_end.device)
    L.check(L.lib().sast_evq_schedule(C.byref(a), next_end.data_ptr(), queue.mode, queue.value, int(first_end_us), W,
                                      None if reset is None else reset.data_ptr(), None if final is None else final.data_ptr(),
                                      ends.data_ptr(), due.data_ptr(), backlog.data_ptr(), _stream()), "evq_schedule")


def export_detections(det: torch.Tensor, n_det: torch.Tensor, ends: torch.Tensor, due: torch.Tensor, records: torch.Tensor,
                      counts: torch.Tensor, truncated: torch.Tensor) -> None:
    """sast_detections_export: the padded detections of `functional.postprocess_padded` (det fp32 [S, A, 7], n_det int32 [S]) of the rows
    with due[s] != 0 (uint8 [S]) -> the first min(n_det[s], max_det) of them as 40-byte records of `labels.BBOX_DTYPE` in records (uint8
    [S, max_det, 40]) with t = ends[s] (int64 [S]), x, y = x1, y1, w, h = x2 - x1, y2 - y1 in fp32, class_id = column 6, track_id = 0,
    class_confidence = column 5; counts int32 [S] is the number written (0 for a row that is not due), truncated (int32 [1]) grows by
    what max_det cut off.  One launch, no synchronisation."""
    F.tensor_arg(det, "det", "online", (torch.float32,), ("S", "A", 7))
    S, A = det.shape[0], det.shape[1]
    F.tensor_arg(records, "records", "online", (torch.uint8,), (S, "max_det", RECORD_BYTES))
    for t, dt, n, name in ((n_det, torch.int32, S, "n_det"), (ends, torch.int64, S, "ends"), (due, torch.uint8, S, "due"),
                           (counts, torch.int32, S, "counts"), (truncated, torch.int32, 1, "truncated")):
        F.tensor_arg(t, name, "online", (dt,), (n,))
    _need_gpu(det, n_det, ends, due, records, counts, truncated)
    a = L.SastDetExportArgs()
    a.det, a.n_det, a.ends, a.due = det.data_ptr(), n_det.data_ptr(), ends.data_ptr(), due.data_ptr()
    a.records, a.counts, a.truncated = records.data_ptr(), counts.data_ptr(), truncated.data_ptr()
    a.S, a.A, a.max_det = S, A, records.shape[1]
    L.check(L.lib().sast_detections_export(C.byref(a), _stream()), "detections_export")


class DetectionLog:
    """log = DetectionLog(num_streams, capacity): the detections of an online run, kept on the device as `PropheseeEvaluator.
    add_recordings` takes them (`dt=log.records, n_dt=log.counts`), so a run is scored without its records visiting the host.
      records int32 [S, capacity, 10] (ten words per `labels.BBOX_DTYPE` record), counts int64 [S], dropped int32 [1]; allocated by the
      first, un-captured `append`.
    log.append(records, counts): sast_detlog_append -- row s puts the counts[s] (int32 [S]) records of one step (uint8 [S, max_det, 40],
      what `export_detections` wrote) behind its log.  A step's records that do not fit are dropped whole and counted in `dropped`.
      One launch, no synchronisation.
    log.clear(streams=None): from the host, the rows `streams` (default: all, and `dropped`) start over.
    A row's log is ONE recording: clear it before the stream is reset.  Otherwise its timestamps go backwards and `add_recordings`
    refuses the row as unsorted -- loudly, in `evaluate_buffer`."""

    def __init__(self, num_streams: int, capacity: int):
        self.num_streams = F.stream_count(num_streams, "online")
        self.capacity = int(capacity)
        if self.capacity < 1 or self.num_streams * self.capacity > (1 << 31) - 1:
            raise ValueError("sast_amd.online: the log's capacity must be >= 1 and num_streams * capacity <= 2^31 - 1")
        self.records = self.counts = self.dropped = None

    def append(self, records: torch.Tensor, counts: torch.Tensor) -> None:
        S = self.num_streams
        F.tensor_arg(records, "records", "online", (torch.uint8,), (("num_streams", S), "max_det", RECORD_BYTES))
        F.tensor_arg(counts, "counts", "online", (torch.int32,), (S,))
        _need_gpu(records, counts)
        F.same_device("online", "records and counts", records, counts)
        if self.records is None:
            F.not_capturing("online", "one un-captured call is needed before graph capture (it allocates the log)")
            dev = records.device
            self.records = torch.zeros(S, self.capacity, RECORD_BYTES // 4, dtype=torch.int32, device=dev)
            self.counts = torch.zeros(S, dtype=torch.int64, device=dev)
            self.dropped = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            F.lives_on("the log", self.records.device, "the step's records", records.device, "online")
        a = L.SastDetLogArgs()
        a.records, a.counts, a.log, a.log_counts, a.dropped = (records.data_ptr(), counts.data_ptr(), self.records.data_ptr(),
                                                               self.counts.data_ptr(), self.dropped.data_ptr())
        a.capacity, a.S, a.max_det = self.capacity, S, records.shape[1]
        L.check(L.lib().sast_detlog_append(C.byref(a), _stream()), "detlog_append")

    def clear(self, streams=None) -> None:
        F.reset_rows((self.counts,), self.dropped, streams, self.num_streams, "online")


class OnlineDetector:
    """od = OnlineDetector(detector, queue, windows_per_step=W, max_det=100, conf_thre=0.1, nms_thre=0.45, first_end_us=None, log=None,
    tracker=None)
      detector: a `YoloXDetector` in eval mode; queue: an `EventQueue` with duration windows (duration_us = D) for S <= 256 streams;
      first_end_us: the end of every recording's first window (default D, must be >= D); log: a `DetectionLog` for the same S
      streams: every step then appends its exported records to it, inside the push (and its graph) -- one more launch per step;
      tracker: a `tracking.DetectionTracker` for the same S streams and at least max_det records: every step then writes the track_id of
      its exported records, in front of the log, inside the push (and its graph) -- one more launch per step.  The tracker follows `reset`;
      its counters are read from the tracker (`tracker.errors()`).
    od.push(x, y, p, t, counts, reset=None, final=None) / od.push_dat(records, counts, reset=None, final=None) /
    od.push_evt3(words, counts, reset=None, final=None) / od.push_evt2(words, counts, reset=None, final=None, version="2.0")
      the chunk of `EventQueue.push` / `push_dat` / `push_evt3` (raw EVT 3.0 sensor words, counts in words) / `push_evt2` (raw EVT 2.0
      or, with version="2.1", EVT 2.1 sensor words, counts in words); reset uint8 / bool [S]:
      the flagged rows start a new recording with this chunk (queue row, recurrent state and schedule start over); final uint8 / bool
      [S]: the flagged recordings are over, their last windows are given although no later event will come.
    od.poll() -> the finished steps' detections, oldest first: a list of (stream, numpy array of `labels.BBOX_DTYPE`), one entry per due
      window (an empty array for a window without detections; `t` of every record is the window's end).  Never waits: steps whose
      copy has not landed stay pending.  od.drain() waits for all of them.
    od.capture() / od.replay(): after one eager push, capture that push (same tensors) as one graph; replay() runs it on the chunk,
      counts and flags written into those tensors since.
    od.errors() -> (invalid events, windows over capacity, dropped events, late windows, detections cut by max_det, windows due but
      not yet given after the last push) (synchronises).

    One push, whatever the data: queue push (2 launches; 4 for push_evt3 / push_evt2, the decode in front; `EventFilter.FILTER_LAUNCHES`
    more and the filter's radix sort with a filtered queue, `EventQueue(filter=...)`); `zero_samples_dev` of the held states
    by `reset`; the schedule (1 launch) -> ends, due [W, S]; `queue.frames(ends)` (7 launches); then for k < W the detector forward on
    frames[k] with the held states, `commit_samples_dev(held, new, due[k])`, `postprocess_padded`, the record export and, where given,
    the tracker's step and the log's append (1 launch each).  A row whose
    window k is not due runs on the frame of the last window it gave and its new (h, c) is dropped, so its state is bit for bit what
    it was.  More than W due windows of a row stay in `backlog` and come out of the following pushes (an empty chunk will do).
    Results: ends, due, counts and records lie in one device buffer that one asynchronous copy moves into one of two pinned host slots,
    with an event behind it.  The copy stays OUTSIDE the captured graph (replay() issues it after the graph), so one graph serves both
    slots.  A third push without a poll in between has no free slot: it waits for the oldest step and keeps its result for the next
    poll.  Otherwise nothing between push and poll synchronises.  The held states (zeros of the shapes a first forward returns), every
    buffer and the slots are allocated by the first, un-captured push and keep their addresses; afterwards only the caching allocator's
    per-call tensors of the detector are taken."""

    def __init__(self, detector, queue: EventQueue, windows_per_step: int, max_det: int = 100, conf_thre: float = 0.1, nms_thre: float = 0.45,
                 first_end_us: Optional[int] = None, class_agnostic: bool = False, log: Optional[DetectionLog] = None,
                 tracker: Optional[DetectionTracker] = None):
        if not isinstance(queue, EventQueue):
            raise ValueError("sast_amd.online: queue must be a sast_amd.events.EventQueue")
        if queue.mode != L.EVENT_WINDOW_DURATION or queue.value < 1:
            raise ValueError("sast_amd.online: OnlineDetector needs a queue with duration windows (duration_us >= 1): count windows have no "
                             "schedule in time")
        if int(windows_per_step) < 1 or int(max_det) < 1:
            raise ValueError("sast_amd.online: windows_per_step and max_det must be >= 1")
        self.queue, self.detector = queue, detector
        self.S, self.W, self.max_det, self.D = queue.num_streams, int(windows_per_step), int(max_det), queue.value
        if self.S > 256:
            raise ValueError("sast_amd.online: at most 256 streams share a batch")
        queue.ws_bytes(self.W * self.S, queue.window_capacity if queue.window_capacity is not None else queue.capacity)   # ValueError
        self.first_end_us = self.D if first_end_us is None else int(first_end_us)
        if self.first_end_us < self.D:
            raise ValueError(f"sast_amd.online: first_end_us must be >= duration_us ({self.D}), got {first_end_us}")
        if getattr(detector, "training", False):
            raise ValueError("sast_amd.online: the detector must be in eval mode (detector.eval())")
        if log is not None and (not isinstance(log, DetectionLog) or log.num_streams != self.S):
            raise ValueError(f"sast_amd.online: log must be a DetectionLog for the queue's {self.S} streams")
        self.log = log
        if tracker is not None and (not isinstance(tracker, DetectionTracker) or tracker.num_streams != self.S or tracker.max_det < self.max_det):
            raise ValueError(f"sast_amd.online: tracker must be a DetectionTracker for the queue's {self.S} streams and max_det >= {self.max_det}")
        self.tracker = tracker
        self.num_classes = int(detector.yolox_head.num_classes)
        self.conf_thre, self.nms_thre, self.class_agnostic = float(conf_thre), float(nms_thre), bool(class_agnostic)
        self.states = None                 # [(h, c)] per stage: the held recurrent states
        self.predictions: List[torch.Tensor] = []   # the decoded head outputs [S, A, 5 + classes] of the last push, one per step
        self.next_end = self.ends = self.due = self.backlog = self.records = self.counts = self.truncated = None
        self._buf = self._frames = None
        self._slots, self._turn, self._pending, self._done = [], 0, [], []
        self._last = self._graph = None

    # ------------------------------------------------------------------------------------------------------------------ buffers
    def _allocate(self, dev: torch.device):
        F.not_capturing("online", "one un-captured call is needed before graph capture (it allocates the buffers)")
        W, S, M = self.W, self.S, self.max_det
        n = W * S
        sizes = (8 * n, RECORD_BYTES * M * n, 4 * n, n)           # ends, records, counts, due: every offset a multiple of 8
        self._offsets = [sum(sizes[:i]) for i in range(5)]
        o = self._offsets
        self._buf = buf = torch.zeros(o[4], dtype=torch.uint8, device=dev)
        self.ends = buf[o[0]:o[1]].view(torch.int64).view(W, S)
        self.records = buf[o[1]:o[2]].view(W, S, M, RECORD_BYTES)
        self.counts = buf[o[2]:o[3]].view(torch.int32).view(W, S)
        self.due = buf[o[3]:o[4]].view(W, S)
        self.next_end = torch.full((S,), self.first_end_us, dtype=torch.int64, device=dev)
        self.backlog = torch.zeros(S, dtype=torch.int64, device=dev)
        self.truncated = torch.zeros(1, dtype=torch.int32, device=dev)
        self._frames = torch.empty((W, S) + self.queue.get_shape(), dtype=self.queue.frame_dtype, device=dev)
        self._slots = [(torch.empty(o[4], dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]

    def _zero_states(self, frame: torch.Tensor):
        """zeros of the shapes and memory layouts a first forward returns"""
        _out, _losses, states, _p = self.detector(frame, None)
        self.states = [(torch.zeros_like(h), torch.zeros_like(c)) for h, c in states]

    # ------------------------------------------------------------------------------------------------------------------ one push
    def _device_step(self, push, counts, reset, final):
        q, S, W = self.queue, self.S, self.W
        F.flags(final, "final", S, "online")
        _need_gpu(final)
        push(counts, reset)                                       # validates the chunk, counts and reset; 2 launches
        if self._buf is None:
            self._allocate(counts.device)
        F.same_device("online", "final and the chunk", final, counts)
        held = None if self.states is None else [t for s in self.states for t in s]
        if held is not None and reset is not None:
            SF.zero_samples_dev(held, reset)
        schedule_windows(q, self.next_end, self.first_end_us, self.ends, self.due, self.backlog, reset, final)
        frames = q.frames(self.ends, out=self._frames)
        if self.states is None:                                   # the first push: its states are zero whatever `reset` says
            self._zero_states(frames[0])
            held = [t for s in self.states for t in s]
        self.predictions = []
        for k in range(W):
            out, _losses, new, _p = self.detector(frames[k], self.states)
            SF.commit_samples_dev(held, [t for s in new for t in s], self.due[k])
            det, n_det = SF.postprocess_padded(out, self.num_classes, self.conf_thre, self.nms_thre, self.class_agnostic)
            export_detections(det, n_det, self.ends[k], self.due[k], self.records[k], self.counts[k], self.truncated)
            if self.tracker is not None:                          # a push is one recording step per row: `reset` acts once, at its first step
                self.tracker.step(self.records[k], self.counts[k], self.ends[k], self.due[k], reset if k == 0 else None)
            if self.log is not None:
                self.log.append(self.records[k], self.counts[k])
            self.predictions.append(out)

    def _copy_out(self):
        host, ev = self._slots[self._turn]
        if any(i == self._turn for i in self._pending):           # no free slot: the oldest step is waited for and kept
            self._harvest(wait=True, only=1)
        host.copy_(self._buf, non_blocking=True)
        ev.record()
        self._pending.append(self._turn)
        self._turn ^= 1

    @torch.no_grad()
    def _step(self, push, tensors, counts, reset, final):
        self._device_step(push, counts, reset, final)
        self._last = (push, tensors, counts, reset, final)        # what capture() captures: the same tensors
        self._copy_out()

    def push(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor,
             reset: Optional[torch.Tensor] = None, final: Optional[torch.Tensor] = None) -> None:
        self._step(lambda c, r: self.queue.push(x, y, p, t, c, r), (x, y, p, t), counts, reset, final)

    def push_dat(self, records: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None,
                 final: Optional[torch.Tensor] = None) -> None:
        self._step(lambda c, r: self.queue.push_dat(records, c, r), (records,), counts, reset, final)

    def push_evt3(self, words: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None,
                  final: Optional[torch.Tensor] = None) -> None:
        self._step(lambda c, r: self.queue.push_evt3(words, c, r), (words,), counts, reset, final)

    def push_evt2(self, words: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None,
                  final: Optional[torch.Tensor] = None, version: str = "2.0") -> None:
        self._step(lambda c, r: self.queue.push_evt2(words, c, r, version=version), (words,), counts, reset, final)

    # ------------------------------------------------------------------------------------------------------------------ graph
    def capture(self) -> None:
        """capture the last push -- its chunk, counts and flag tensors -- as one graph.  Capturing runs nothing: the state is untouched."""
        if self._last is None or self._buf is None:
            raise RuntimeError("sast_amd.online: one un-captured call is needed before graph capture (it allocates the buffers)")
        push, _tensors, counts, reset, final = self._last
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._device_step(push, counts, reset, final)
        self._graph = g

    def replay(self) -> None:
        if self._graph is None:
            raise RuntimeError("sast_amd.online: nothing was captured: call capture() after one eager push")
        self._graph.replay()
        self._copy_out()

    # ------------------------------------------------------------------------------------------------------------------ results
    def _parse(self, host: torch.Tensor) -> List[Tuple[int, np.ndarray]]:
        W, S, M, o = self.W, self.S, self.max_det, self._offsets
        raw = host.numpy()
        records = raw[o[1]:o[2]].reshape(W, S, M * RECORD_BYTES)
        counts = raw[o[2]:o[3]].view(np.int32).reshape(W, S)
        due = raw[o[3]:o[4]].reshape(W, S)
        # copied as bytes: numpy copies a structured array field by field and would leave the four padding bytes of a record undefined
        return [(s, records[k, s, :counts[k, s] * RECORD_BYTES].copy().view(BBOX_DTYPE)) for k in range(W) for s in range(S) if due[k, s]]

    def _harvest(self, wait: bool, only: Optional[int] = None):
        n = 0
        while self._pending and (only is None or n < only):
            host, ev = self._slots[self._pending[0]]
            if wait:
                ev.synchronize()
            elif not ev.query():
                break
            self._done.extend(self._parse(host))
            self._pending.pop(0)
            n += 1

    def poll(self) -> List[Tuple[int, np.ndarray]]:
        """the detections of the steps whose copy has landed (never waits)"""
        self._harvest(wait=False)
        out, self._done = self._done, []
        return out

    def drain(self) -> List[Tuple[int, np.ndarray]]:
        """the detections of every step pushed so far (waits for their copies)"""
        self._harvest(wait=True)
        out, self._done = self._done, []
        return out

    def errors(self) -> Tuple[int, int, int, int, int, int]:
        """(invalid events, windows over capacity, dropped events, late windows, detections cut by max_det, windows still in the
        backlog after the last push) (synchronises)"""
        if self._buf is None:
            return (0, 0, 0, 0, 0, 0)
        return tuple(self.queue.errors()) + (int(self.truncated.item()), int(self.backlog.sum().item()))
