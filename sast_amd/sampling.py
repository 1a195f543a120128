"""Random-access training sequences on the GPU (csrc/k_sampler.hip, and the row-mapped window search of csrc/k_events.hip).

The reference trains with `dataset.train.sampling: 'mixed'`: half of the batches are streamed recordings, the other half random-access
samples -- `sequence_length` consecutive windows that end at a randomly chosen label frame (data/genx_utils/sequence_rnd.py,
dataset_rnd.py), every one a first sample of its own (`is_first_sample = True`), with zoom-in placed on the most recent non-empty label
frame (data/utils/augmentor.py:367-378).  `RandomAccessPool` is that second half for R recordings resident in device memory: the item
index of `SequenceForRandomAccess` + `ConcatDataset`, the weights of `get_weighted_random_sampler`, the label tensors of an item, and its
event frames, from raw events and the `LabelStreams` schedule, without the host touching an event or a box.

The pool is a shuffle buffer over the recordings that are resident, not the whole dataset: N, the cumulative sizes and the weights
(whose class totals run over the pool's items) describe the R rows loaded now.  A caller that wants the reference's global shuffle
rotates recordings through the rows (`labels.load(..., reset=)`, `load_events(..., reset=)`, `index()`).

The draws stay on the host, as the augmentor's do, with the calls torch's samplers make:

    n, _ = pool.index()
    items = torch.randperm(n)                                                  # RandomSampler
    n, _ = pool.index(weighted=True)
    items = torch.multinomial(pool.weights[:n].cpu(), n, replacement=True)     # WeightedRandomSampler

`MixedPool` merges both halves into the reference's actual training batch (csrc/k_mixed.hip): Bs streamed rows and Br random-access
samples in one batch, made by one launch, with one frames call over the union.

`StreamingPool` is the first half for the same resident recordings (csrc/k_stream.hip): the sub-sequences of
`SequenceForIter.get_sequences_with_guaranteed_labels`, their samples of `sequence_length` windows with the padded tail, and the
per-batch-row concatenations of `ConcatStreamingDataPipe` (train) / `ShardedStreamingDataPipe` (val / test), walked by a cursor in
device memory so that a captured step is simply replayed to move along the streams.  Its draws stay torch's too (`concat_orders`).

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _frontend as F
from . import _lib as L
from .events import _Windowed
from .functional import _need_gpu, _stream
from .labels import LabelStreams

# status bits (include/sast_hip.h, SAST_RND_*): per row, then pool-wide
ROW_FLAGS = ((L.RND_CLASS_ID, "class_id", "a box of a counted label frame has a class id outside [0, max_classes); it was left out"),)
POOL_FLAGS = ((L.RND_ITEM_INDEX, "item_index", "batch() was given an item outside [0, N)"),)
# status bits of a StreamingPool (SAST_STREAM_*): pool-wide
STREAM_FLAGS = ((L.STREAM_TRUNCATED, "truncated", "more than max_sequences sequences; the table holds the first max_sequences"),
                (L.STREAM_SCHEDULE_INDEX, "schedule_index", "next() met a schedule entry outside [0, n_seq); it gave a fully padded sample"))


class RandomAccessBatch(NamedTuple):
    """what `RandomAccessPool.batch` returns (L = sequence_length, M = the labels' max_labels_per_frame)"""
    rows: torch.Tensor            # int32 [B]: the pool row of every sample, -1 for an item outside [0, N)
    window_idx: torch.Tensor      # int64 [L, B]
    ends_us: torch.Tensor         # int64 [L, B]
    labels: torch.Tensor          # fp32 [L, B, M, 7]
    counts: torch.Tensor          # int32 [L, B]
    labelled: torch.Tensor        # uint8 [L, B]
    latest: torch.Tensor          # fp32 [B, M, 7]
    latest_count: torch.Tensor    # int32 [B]


class RandomAccessLatest(NamedTuple):
    """what `RandomAccessPool.latest` returns: the two zoom-in fields of a `RandomAccessBatch` alone"""
    latest: torch.Tensor          # fp32 [B, M, 7]
    latest_count: torch.Tensor    # int32 [B]


class _PoolEvents(_Windowed):
    """what `RandomAccessPool` and `StreamingPool` share: the resident event columns of R recordings with their timestamps corrected
    once (`load_events`), and the frames of windows that are found through a row map (`_mapped_frames`).  Made with events=, it is a
    frames driver over another pool's events: that pool's columns, corrected timestamps and counts, read by reference, with a
    workspace, window bounds and error counters of its own (`StreamingPool(events=)`, and the union batch of `MixedPool`)."""

    _module = "sampling"

    def __init__(self, labels, height, width, sequence_length, bins, count_cutoff, fastmode, duration_us, downsample_by_2, representation,
                 window_capacity, events=None, events_name="the pool given as events="):
        if not isinstance(labels, LabelStreams):
            raise TypeError("sast_amd.sampling: labels must be a LabelStreams")
        if duration_us is None:
            raise ValueError("sast_amd.sampling: duration_us is required (the windows of a label schedule are duration windows)")
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2, representation, duration_us, None, True,
                         window_capacity)
        if isinstance(sequence_length, bool) or not isinstance(sequence_length, int) or not 1 <= sequence_length <= 65535:
            raise ValueError("sast_amd.sampling: sequence_length must be an int in 1 .. 65535")
        if bool(labels.downsample_by_2) != bool(downsample_by_2):
            raise ValueError("sast_amd.sampling: labels.downsample_by_2 and downsample_by_2 must agree")
        if events is not None and not isinstance(events, _PoolEvents):
            raise TypeError("sast_amd.sampling: events must be a RandomAccessPool or a StreamingPool")
        if events is not None and events.num_rows != labels.num_streams:
            raise ValueError(f"sast_amd.sampling: events holds {events.num_rows} rows, the labels {labels.num_streams}")
        while events is not None and events._events is not None:          # a pool that shares itself: read its source
            events = events._events
        self._events, self._events_name = events, events_name
        self.labels = labels
        self.num_rows = labels.num_streams
        self.sequence_length = sequence_length
        self.x = self.y = self.p = self.t = self.counts = None
        self._codes = None
        self._args = None
        self._host = None          # host mirrors of the last index()

    # ---- events
    def load_events(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor,
                    reset: Optional[torch.Tensor] = None) -> None:
        if self._events is not None:
            raise RuntimeError("sast_amd.sampling: this pool reads the events of the pool given as events=; load them there")
        R = self.num_rows
        codes = F.event_columns(x, y, p, t, R, "sampling", rows_name="rows")
        F.counts_reset(counts, reset, R, "sampling")
        cap = x.shape[1]
        if cap < 1 or R * cap > 2 ** 31 - 1:
            raise ValueError("sast_amd.sampling: capacity must be >= 1 and rows * capacity below 2^31")
        _need_gpu(x, y, p, t, counts, reset)
        dev = x.device
        F.same_device("sampling", "x, y, p, t, counts and reset", x, y, p, t, counts, reset)
        if self.t is None or self.t.device != dev or self.t.shape[1] != cap:
            F.not_capturing("sampling")
            self.t = torch.zeros(R, cap, dtype=torch.int64, device=dev)
            self.counts = torch.zeros(R, dtype=torch.int64, device=dev)
            self.t_last = None
            self._carry(dev, (R,))
            self._state = {"scan": torch.empty(int(L.lib().sast_evstreams_ws_count(R)), dtype=torch.int64, device=dev),
                           "ones": torch.ones(R, dtype=torch.uint8, device=dev)}
            if reset is not None:
                reset = None           # nothing to keep: every row is new
        st = self._state
        if reset is None:
            now, flags = counts, st["ones"]
            self.counts.copy_(counts)
        else:
            keep = reset == 0
            now, flags = counts.masked_fill(keep, 0), reset          # a row that is kept: no event, so nothing of it is rewritten
            self.counts.copy_(torch.where(keep, self.counts, counts))
        L.check(L.lib().sast_evstreams_correct_time(t.data_ptr(), codes[3], now.data_ptr(), R, cap, self.t.data_ptr(), self.t_last.data_ptr(),
                                                    flags.data_ptr(), st["scan"].data_ptr(), _stream()), "evstreams_correct_time")
        self.x, self.y, self.p = x, y, p
        self._codes = codes[:3] + [L.DT_I64]

    def frame_errors(self) -> Tuple[int, int]:
        """(invalid events, windows over capacity) of the frames calls since the pool was made (synchronises)"""
        return _Windowed.errors(self)

    def _source(self) -> "_PoolEvents":
        """the pool whose loaded events this one's frames read: itself, or the one it was made over"""
        src = self._events if self._events is not None else self
        if src.x is None:
            raise RuntimeError("sast_amd.sampling: call load_events() before frames()" + (f" (on {self._events_name})" if src is not self else ""))
        return src

    def _label_elems_guard(self, B: int) -> None:
        """the label tensors of a batch of B columns are indexed in 32 bits, eight floats a row"""
        if B * self.sequence_length * self.labels.max_labels_per_frame > (2 ** 31 - 1) // 8:
            raise ValueError("sast_amd.sampling: B * sequence_length * max_labels_per_frame must be <= (2^31 - 1) / 8")

    def _step_frames(self, batch, out_frames: Optional[torch.Tensor]) -> torch.Tensor:
        """the frames of a batch that carries its row map per step (`step_rows` int32 [L, B], `ends_us` int64 [L, B]): every (step,
        column) is a window of its own with its own row; a padded step's row is -1, which gives the empty range"""
        step_rows, ends = batch.step_rows, batch.ends_us
        _need_gpu(step_rows, ends, out_frames)
        src = self._source()
        Ls = self.sequence_length
        F.tensor_arg(step_rows, "batch.step_rows", "sampling", (torch.int32,), (Ls, "B"))
        B = step_rows.shape[1]
        F.tensor_arg(ends, "batch.ends_us", "sampling", (torch.int64,), (Ls, B))
        dev = src.t.device
        if self.err is None or self.err.device != dev:            # a pool that reads another pool's events keeps its own counters
            F.not_capturing("sampling")
            self.err = torch.zeros(2, dtype=torch.int32, device=dev)
        return self._mapped_frames(src, step_rows, Ls * B, 1, ends, (Ls, B) + self.get_shape(), out_frames)

    def _mapped_frames(self, src, row_map: torch.Tensor, cols: int, T: int, ends: torch.Tensor, shape, out_frames):
        """the frames of the T * cols windows ends[k, c] searched in row row_map[c] of `src`'s events (1 + 4 launches)"""
        R, cap = self.num_rows, src.t.shape[1]
        wcap = self.window_capacity if self.window_capacity is not None else cap
        self.ws_bytes(T * cols, wcap)             # ValueError for more windows than the histogram kernels take
        dev = src.t.device
        for t in (row_map, ends):
            F.lives_on("the pool's event storage", dev, "the batch", t.device, "sampling")
        out_frames = F.frames_out(out_frames, shape, self.frame_dtype, dev, "sampling", "out_frames", "the events'")
        bounds = self._bounds(T * cols, dev, "batch size")
        L.check(L.lib().sast_rnd_window_bounds(src.t.data_ptr(), src.counts.data_ptr(), R, cap, row_map.data_ptr(), ends.data_ptr(),
                                                          cols, T, self.mode, self.value, bounds.data_ptr(), _stream()),
                "rnd_window_bounds")
        self.launch([src.x, src.y, src.p, src.t], src._codes, R * cap, bounds, out_frames, self.err, wcap, clip_negative_polarity=True)
        self.last_bounds = bounds
        return out_frames


class RandomAccessPool(_PoolEvents):
    """pool = RandomAccessPool(labels, height, width, sequence_length=L, only_load_end_labels=False, bins=10, count_cutoff=10,
                               fastmode=True, duration_us=50_000, downsample_by_2=False, representation="stacked_histogram",
                               window_capacity=None, max_classes=16)
    pool.load_events(x, y, p, t, counts, reset=None)
    n, cumulative_sizes = pool.index(weighted=False)
    out = pool.batch(items, out=None)
    frames = pool.frames(out, out_frames=None)
    latest, latest_count = pool.latest(items, out=None)
    pool.labelled_pairs(items_host); pool.errors()

    labels: a `LabelStreams` of R rows the caller has `load`ed (or loads before `index`): row r's box records and row r's events are
      one recording.  The geometry arguments are `EventStreams`'.
    load_events: x, y, p, t contiguous [R, cap] device tensors (dtypes as in `EventStreams`), counts int64 [R].  The pool keeps the
      columns by reference (they must stay as they are while batches are drawn) and corrects the timestamps of the rows with
      reset[r] != 0 (uint8 / bool [R]; default: every row) once, from a carry of 0, into its own int64 [R, cap] buffer `t`; the other
      rows keep the corrected timestamps and the count they have.  2 launches.
    index: after `labels.load`.  Device state: start_idx_offset, length int32 [R], cum int64 [R + 1] (cum[0] = 0), and with weighted=True
      class_total int64 [max_classes] and weights fp64 [R * max_frames] (item g at [g], zeros behind N).  Returns N = cum[R] and
      ConcatDataset's cumulative_sizes (cum[1:], a list) through ONE synchronising copy.  1 launch, 3 with weighted=True.  It clears
      the status words.
    batch: items int64 [B] on the device (ConcatDataset indices) -> `RandomAccessBatch`.  Item g lies in the row r with
      cum[r] <= g < cum[r + 1]; its label frame is j = g - cum[r] + start_idx_offset[r], its windows are frame_2_window[r][j] + 1 - L ...
      frame_2_window[r][j].  labels / counts / ends_us / labelled of step k and sample b are what `LabelStreams.labels` gives for row
      rows[b] at window_idx[k, b]; with only_load_end_labels the steps before the last have counts 0, labelled 0 and zero rows (the
      reference puts None there), ends_us is still filled.  latest[b] / latest_count[b]: the rows of the sample's last step with
      counts > 0, unaugmented (get_most_recent_objframe(check_if_nonempty=True)); latest_count 0: none.  The copy of `latest` to the
      host for `SpatialAugmentor.randomize(latest_labels=)` is the caller's, one per batch.  An item outside [0, N): rows -1,
      window_idx and ends_us -1, counts 0, zero frames, and item_index in the pool's status.  Two samples of one row are allowed.
      1 launch.
    frames: the batch's event frames, [L, B, C, H', W'] uint8 (int8 for mixed_density): frames[k, b] is byte for byte what an
      `EventStreams(num_streams=R, ...same arguments...)` gives for row rows[b] at window end ends_us[k, b] on the same columns with
      reset all ones.  5 launches (1 window search through the row map, 4 histogram).  window_capacity: kept events one window may
      hold (default: cap); `err` / `frame_errors()` as `EventStreams.errors()`.
    latest: items as for batch -> `RandomAccessLatest`: latest / latest_count alone, bit for bit what batch gives for the same items
      (the look-ahead of `MixedPool.prefetch_latest`).  1 launch, a workgroup per sample.
    labelled_pairs: host only -- the number K of labelled (step, sample) pairs of a batch of items (the batch of the PAFPN / head pass,
      `TrainStep(selection=)`), from the host mirrors of `index()` and `labels.labelled_windows()` (fetched once after each `index`).
    errors: (per row the names of its status bits, the names of the pool's) (synchronises).
    After one un-captured call of batch and frames with the same B nothing is allocated but the outputs and nothing synchronises:
    batch + frames (+ augmentor + backbone) can be captured in one graph and replayed with new items written into the same tensor.
    Limits: the pool covers the resident recordings only; R * cap must stay below 2^31."""

    LOAD_EVENTS_LAUNCHES = 2
    INDEX_LAUNCHES = 1
    INDEX_WEIGHTED_LAUNCHES = 3
    BATCH_LAUNCHES = 1
    LATEST_LAUNCHES = 1
    FRAMES_LAUNCHES = 5

    def __init__(self, labels: LabelStreams, height: int, width: int, sequence_length: int, only_load_end_labels: bool = False,
                 bins: int = 10, count_cutoff: Optional[int] = 10, fastmode: bool = True, duration_us: int = 50_000,
                 downsample_by_2: bool = False, representation: str = "stacked_histogram", window_capacity: Optional[int] = None,
                 max_classes: int = 16):
        super().__init__(labels, height, width, sequence_length, bins, count_cutoff, fastmode, duration_us, downsample_by_2, representation,
                         window_capacity)
        if isinstance(max_classes, bool) or not isinstance(max_classes, int) or not 1 <= max_classes <= L.RND_MAX_CLASSES:
            raise ValueError(f"sast_amd.sampling: max_classes must be an int in 1 .. {L.RND_MAX_CLASSES}")
        self.only_load_end_labels, self.max_classes = bool(only_load_end_labels), max_classes
        self.start_idx_offset = self.length = self.cum = self.class_total = self.weights = self.status = None
        # _host: (cum [R + 1], start_idx_offset [R]) as numpy, from the last index()
        self._labelled = None      # labels.labelled_windows() of that index, and per row the window of every label frame

    # ---- the item index
    def _storage(self, dev):
        if self._args is None:
            F.not_capturing("sampling")
            R, Fr = self.num_rows, self.labels.max_frames
            self.start_idx_offset, self.length = (torch.zeros(R, dtype=torch.int32, device=dev) for _ in range(2))
            self.cum = torch.zeros(R + 1, dtype=torch.int64, device=dev)
            self.class_total = torch.zeros(self.max_classes, dtype=torch.int64, device=dev)
            self.weights = torch.zeros(R * Fr, dtype=torch.float64, device=dev)
            self.status = torch.zeros(R + 1, dtype=torch.int32, device=dev)
            self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            a = self._args = L.SastRndArgs()
            a.start_idx_offset, a.length, a.cum = self.start_idx_offset.data_ptr(), self.length.data_ptr(), self.cum.data_ptr()
            a.class_total, a.weights, a.status = self.class_total.data_ptr(), self.weights.data_ptr(), self.status.data_ptr()
            a.ticket = self._ticket.data_ptr()
            a.sequence_length, a.only_load_end_labels, a.max_classes = self.sequence_length, int(self.only_load_end_labels), self.max_classes
        return self._args

    def index(self, weighted: bool = False) -> Tuple[int, List[int]]:
        if self.labels._args is None:
            raise RuntimeError("sast_amd.sampling: call labels.load() before index()")
        a = self._storage(self.labels.status.device)
        a.weighted = int(bool(weighted))
        L.check(L.lib().sast_rnd_index(C.byref(self.labels._args), C.byref(a), _stream()), "rnd_index")
        R = self.num_rows
        both = torch.cat([self.cum, self.start_idx_offset.to(torch.int64)]).cpu().numpy()
        self._host = (both[:R + 1].copy(), both[R + 1:].copy())
        self._labelled = None
        return int(both[R]), [int(v) for v in both[1:R + 1]]

    def errors(self) -> Tuple[List[Tuple[str, ...]], Tuple[str, ...]]:
        if self.status is None:
            return [()] * self.num_rows, ()
        v = [int(s) for s in self.status.tolist()]
        return ([tuple(n for bit, n, _m in ROW_FLAGS if s & bit) for s in v[:-1]], tuple(n for bit, n, _m in POOL_FLAGS if v[-1] & bit))

    # ---- batches
    def _want(self, B: int):
        Ls, M = self.sequence_length, self.labels.max_labels_per_frame
        return (((B,), torch.int32), ((Ls, B), torch.int64), ((Ls, B), torch.int64), ((Ls, B, M, 7), torch.float32), ((Ls, B), torch.int32),
                ((Ls, B), torch.uint8), ((B, M, 7), torch.float32), ((B,), torch.int32))

    def batch(self, items: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> RandomAccessBatch:
        B, dev = self._items(items), items.device
        self._label_elems_guard(B)
        out = F.outputs(RandomAccessBatch, self._want(B), out, dev, "sampling", "eight tensors of a RandomAccessBatch", "the pool's")
        L.check(L.lib().sast_rnd_gather(C.byref(self.labels._args), C.byref(self._args), items.data_ptr(), B, *(t.data_ptr() for t in out),
                                        _stream()), "rnd_gather")
        return out

    def _items(self, items: torch.Tensor) -> int:
        F.tensor_arg(items, "items", "sampling", (torch.int64,), ("B",))
        _need_gpu(items)
        if self._args is None:
            raise RuntimeError("sast_amd.sampling: call index() before batch() / latest()")
        F.lives_on("the pool", self.status.device, "items", items.device, "sampling")
        return items.numel()

    def latest(self, items: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> RandomAccessLatest:
        B = self._items(items)
        M = self.labels.max_labels_per_frame
        if B * M > (2 ** 31 - 1) // 8:
            raise ValueError("sast_amd.sampling: B * max_labels_per_frame must be <= (2^31 - 1) / 8")
        out = F.outputs(RandomAccessLatest, (((B, M, 7), torch.float32), ((B,), torch.int32)), out, items.device, "sampling",
                        "two tensors of a RandomAccessLatest", "the pool's")
        L.check(L.lib().sast_mixed_latest(C.byref(self.labels._args), C.byref(self._args), items.data_ptr(), B, out.latest.data_ptr(),
                                          out.latest_count.data_ptr(), _stream()), "mixed_latest")
        return out

    def frames(self, batch: RandomAccessBatch, out_frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        rows, ends = batch.rows, batch.ends_us
        _need_gpu(rows, ends, out_frames)
        src, Ls = self._source(), self.sequence_length
        F.tensor_arg(rows, "batch.rows", "sampling", (torch.int32,), ("B",))
        B = rows.numel()
        F.tensor_arg(ends, "batch.ends_us", "sampling", (torch.int64,), (Ls, B))
        return self._mapped_frames(src, rows, B, Ls, ends, (Ls, B) + self.get_shape(), out_frames)

    def labelled_pairs(self, items_host) -> int:
        if self._host is None:
            raise RuntimeError("sast_amd.sampling: call index() before labelled_pairs()")
        if isinstance(items_host, torch.Tensor):
            if items_host.is_cuda:
                raise ValueError("sast_amd.sampling: labelled_pairs takes the items on the host (the draw is made there)")
            items_host = items_host.numpy()
        items = np.asarray(items_host, dtype=np.int64).reshape(-1)
        cum, offset = self._host
        if self._labelled is None:
            lw = self.labels.labelled_windows()
            self._labelled = (lw, [np.flatnonzero(w) for w in lw])
        lw, f2w = self._labelled
        Ls, K = self.sequence_length, 0
        for g in items.tolist():
            if not 0 <= g < cum[-1]:
                continue
            r = int(np.searchsorted(cum[1:], g, side="right"))
            end = int(f2w[r][g - int(cum[r]) + int(offset[r])]) + 1
            K += 1 if self.only_load_end_labels else int(lw[r][end - Ls:end].sum())
        return K


class StreamingBatch(NamedTuple):
    """what `StreamingPool.next` returns (L = sequence_length, M = the labels' max_labels_per_frame)"""
    rows: torch.Tensor            # int32 [B]: the pool row (recording) of every batch row, -1: exhausted or a bad schedule entry
    step_rows: torch.Tensor       # int32 [L, B]: `rows` on a real step, -1 on a padded one (the row map of the frames)
    seq: torch.Tensor             # int32 [B]: the sequence, -1 as for rows
    sample: torch.Tensor          # int32 [B]: the sample inside the sequence, -1 as for rows
    is_first: torch.Tensor        # uint8 [B]: sample == 0 (reset the recurrent states of this row)
    exhausted: torch.Tensor       # uint8 [B]: the row's schedule is used up
    window_idx: torch.Tensor      # int64 [L, B], -1 on padded steps
    ends_us: torch.Tensor         # int64 [L, B], -1 on padded steps
    labels: torch.Tensor          # fp32 [L, B, M, 7]
    counts: torch.Tensor          # int32 [L, B]
    labelled: torch.Tensor        # uint8 [L, B]
    is_padded: torch.Tensor       # uint8 [L, B]


class StreamingPlan(NamedTuple):
    """what `StreamingPool.plan` returns, host arrays over the steps('longest') steps of the schedule"""
    K: np.ndarray                 # int64 [n_steps]: labelled (step, sample) pairs of the batch
    is_first: np.ndarray          # bool [n_steps, B]
    seq: np.ndarray               # int32 [n_steps, B], -1: the row is exhausted


def _pyramid(n: int):
    """ShardedStreamingDataPipe.yield_pyramid_indices(0, n): 0 .. n-1, n-1 .. 0, 0 .. n-1, ..."""
    while True:
        yield from range(n)
        yield from range(n - 1, -1, -1)


class StreamingPool(_PoolEvents):
    """pool = StreamingPool(labels, height, width, sequence_length=L, guarantee_labels=True, events=None, max_sequences=None,
                            order_capacity=None, bins=10, count_cutoff=10, fastmode=True, duration_us=50_000, downsample_by_2=False,
                            representation="stacked_histogram", window_capacity=None)
    pool.load_events(x, y, p, t, counts, reset=None)          (not with events=)
    n_seq, sequences = pool.index(check=False)
    pool.set_schedule(pool.concat_orders(B))                  or pool.sharded_orders(B, total_num_workers, global_worker_id)
    K, is_first, seq = pool.plan(); pool.steps('shortest' | 'longest')
    out = pool.next(out=None)
    frames = pool.frames(out, out_frames=None)
    pool.errors(); pool.frame_errors()

    labels: a `LabelStreams` of R rows, as for `RandomAccessPool`; the geometry arguments are `EventStreams`'.
    guarantee_labels: True -- the training split: `SequenceForIter.get_sequences_with_guaranteed_labels`, a recording is cut wherever
      two label frames lie more than L windows apart; False -- validation / test: one sequence per recording, from L - 1 windows before
      its first label frame to its last window.
    events: a `RandomAccessPool` or `StreamingPool` over the same R rows whose `load_events` columns, corrected timestamps and counts
      this pool reads by reference: in mixed mode the recordings are loaded and time-corrected once.  Without it `load_events` is
      `RandomAccessPool.load_events` (2 launches).
    index: after `labels.load`.  Device state: seq_row, seq_start, seq_stop, seq_samples int32 [max_sequences] (default R * max_frames
      with guarantee_labels, else R), row_first_seq int32 [R + 1], n_seq int32 [1].  Sequences are numbered row-major, in ascending
      window order inside a row (`datapipes.extend(new_datapipes)` over the recordings); a row without frames (a flagged row of
      `LabelStreams`) has none.  Returns n_seq and `sequences`, numpy int32 [n_seq, 4] = (row, start, stop, samples), through ONE
      synchronising copy that also brings the host mirrors `plan` needs.  2 launches.  It clears the status words; check=True raises
      ValueError naming the status bits.
    concat_orders / sharded_orders: host only -- B lists of sequence ids.  concat: B times `torch.randperm(n_seq)`, drawn in batch-row
      order (`ConcatStreamingDataPipe._get_zipped_streams`).  sharded: `ShardedStreamingDataPipe` -- the stable long-to-short sort by
      samples, the pyramid deal to workers, the second sort, the pyramid deal to batch rows; ValueError where the reference asserts.
    set_schedule: B sequences of ids, validated on the host against n_seq and order_capacity (default max_sequences) -> order int32
      [B, order_capacity], order_len int32 [B] and zeroed cursors int32 [B, 2] by stream-ordered copies into tensors that keep their
      place while B stays the same (a captured `next` follows a new schedule).
    plan: host only, no sync -- per step K (section 3f's K), is_first [n_steps, B] and seq [n_steps, B] over steps('longest') steps.
      steps('shortest'): the training Zipper (the epoch ends when the first row runs out); steps('longest'): ZipperLongest.
    next: -> `StreamingBatch`, then every row's cursor moves on by one sample.  Sample i of sequence s: step k is window
      seq_start[s] + i * L + k, padded from seq_stop[s] on.  labels / counts / ends_us / labelled of a real step are what
      `LabelStreams.labels` gives for row rows[b] at window_idx[k, b]; a padded step has window_idx and ends_us -1, zeros elsewhere and
      is_padded 1 (the reference puts None and the padding representation there).  A row whose schedule is used up gives
      get_fully_padded_sample: rows -1, is_first 0, exhausted 1, every step padded, and its cursor stays.  A schedule entry outside
      [0, n_seq) (only a schedule written past set_schedule can hold one) gives the same with exhausted 0, sets schedule_index and is
      skipped.  1 launch, a workgroup per batch row.
    frames: [L, B, C, H', W'] uint8 (int8 for mixed_density): a real step is byte for byte what `EventStreams` gives for that row and
      window end; a padded step is all zero whatever the timestamps are (its row in the row map is -1).  5 launches.
    After one un-captured call of next and frames with the same B nothing is allocated but the outputs and nothing synchronises:
    next + frames (+ augmentor + step) are captured in one graph, and every replay advances the streams.
    Limits: the pool covers the resident recordings only; R * cap must stay below 2^31."""

    LOAD_EVENTS_LAUNCHES = 2
    INDEX_LAUNCHES = 2
    NEXT_LAUNCHES = 1
    FRAMES_LAUNCHES = 5

    def __init__(self, labels: LabelStreams, height: int, width: int, sequence_length: int, guarantee_labels: bool = True,
                 events: Optional[_PoolEvents] = None, max_sequences: Optional[int] = None, order_capacity: Optional[int] = None,
                 bins: int = 10, count_cutoff: Optional[int] = 10, fastmode: bool = True, duration_us: int = 50_000,
                 downsample_by_2: bool = False, representation: str = "stacked_histogram", window_capacity: Optional[int] = None):
        super().__init__(labels, height, width, sequence_length, bins, count_cutoff, fastmode, duration_us, downsample_by_2, representation,
                         window_capacity, events=events)
        R = self.num_rows
        if max_sequences is None:
            max_sequences = R * labels.max_frames if guarantee_labels else R
        if isinstance(max_sequences, bool) or not isinstance(max_sequences, int) or not 1 <= max_sequences <= 2 ** 31 - 1:
            raise ValueError("sast_amd.sampling: max_sequences must be an int in 1 .. 2^31 - 1")
        if order_capacity is None:
            order_capacity = max_sequences
        if isinstance(order_capacity, bool) or not isinstance(order_capacity, int) or not 1 <= order_capacity <= 2 ** 31 - 1:
            raise ValueError("sast_amd.sampling: order_capacity must be an int in 1 .. 2^31 - 1")
        self.guarantee_labels = bool(guarantee_labels)
        self.max_sequences, self.order_capacity = max_sequences, order_capacity
        self.seq_row = self.seq_start = self.seq_stop = self.seq_samples = self.row_first_seq = self.n_seq = self.status = None
        self.order = self.order_len = self.cursor = None
        # _host: (sequences [n_seq, 4], per row the labelled windows) as numpy, from the last index()
        self._orders = None        # the schedule of the last set_schedule()

    # ---- the sequence table
    def _storage(self, dev):
        if self._args is None:
            F.not_capturing("sampling")
            R, n = self.num_rows, self.max_sequences
            self._table = torch.zeros(4, n, dtype=torch.int32, device=dev)
            self.seq_row, self.seq_start, self.seq_stop, self.seq_samples = self._table.unbind(0)
            self.row_first_seq = torch.zeros(R + 1, dtype=torch.int32, device=dev)
            self._row_count = torch.zeros(R, dtype=torch.int32, device=dev)
            self._head = torch.zeros(2, dtype=torch.int32, device=dev)          # n_seq, status: one word each, fetched together
            self.n_seq, self.status = self._head[0:1], self._head[1:2]
            a = self._args = L.SastStreamArgs()
            a.seq_row, a.seq_start, a.seq_stop, a.seq_samples = (t.data_ptr() for t in self._table.unbind(0))
            a.row_first_seq, a.row_count = self.row_first_seq.data_ptr(), self._row_count.data_ptr()
            a.n_seq, a.status = self.n_seq.data_ptr(), self.status.data_ptr()
            a.sequence_length, a.guarantee_labels = self.sequence_length, int(self.guarantee_labels)
            a.max_sequences, a.order_capacity = self.max_sequences, self.order_capacity
        return self._args

    def index(self, check: bool = False) -> Tuple[int, np.ndarray]:
        ls = self.labels
        if ls._args is None:
            raise RuntimeError("sast_amd.sampling: call labels.load() before index()")
        a = self._storage(ls.status.device)
        L.check(L.lib().sast_stream_index(C.byref(ls._args), C.byref(a), _stream()), "stream_index")
        R, n_max = self.num_rows, self.max_sequences
        both = torch.cat([self._head, self._table.reshape(-1), ls.n_windows, ls.window_2_frame.reshape(-1)]).cpu().numpy()
        n, status = int(both[0]), int(both[1])
        table = both[2:2 + 4 * n_max].reshape(4, n_max)
        rest = both[2 + 4 * n_max:]
        n_windows, w2f = rest[:R], rest[R:].reshape(R, ls.max_windows)
        sequences = np.ascontiguousarray(table[:, :n].T)
        self._host = (sequences, [w2f[r, :int(n_windows[r])] >= 0 for r in range(R)])
        self._orders = None
        if check and status:
            raise ValueError("sast_amd.sampling: " + "; ".join(f"{name}: {msg}" for bit, name, msg in STREAM_FLAGS if status & bit))
        return n, sequences

    def errors(self) -> Tuple[str, ...]:
        """the names of the pool's status bits (synchronises)"""
        if self.status is None:
            return ()
        v = int(self.status.item())
        return tuple(n for bit, n, _m in STREAM_FLAGS if v & bit)

    # ---- schedules (host only)
    def _sequences(self) -> np.ndarray:
        if self._host is None:
            raise RuntimeError("sast_amd.sampling: call index() before the schedule methods")
        return self._host[0]

    def concat_orders(self, batch_size: int) -> List[List[int]]:
        n = len(self._sequences())
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError("sast_amd.sampling: batch_size must be an int >= 1")
        return [torch.randperm(n).tolist() for _ in range(batch_size)]

    def sharded_orders(self, batch_size: int, total_num_workers: int = 1, global_worker_id: int = 0) -> List[List[int]]:
        samples = self._sequences()[:, 3].tolist()
        for v, name in ((batch_size, "batch_size"), (total_num_workers, "total_num_workers")):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"sast_amd.sampling: {name} must be an int >= 1")
        if not len(samples) >= total_num_workers > global_worker_id >= 0:
            raise ValueError(f"sast_amd.sampling: {len(samples)} sequences for {total_num_workers} workers (worker {global_worker_id}): "
                             "every worker needs a sequence")
        ids = sorted(range(len(samples)), key=lambda s: samples[s], reverse=True)        # stable: long to short
        mine = [s for s, w in zip(ids, _pyramid(total_num_workers)) if w == global_worker_id]
        if len(mine) < batch_size:
            raise ValueError(f"sast_amd.sampling: worker {global_worker_id} gets {len(mine)} sequences, fewer than batch_size = "
                             f"{batch_size}; decrease the number of workers")
        mine = sorted(mine, key=lambda s: samples[s], reverse=True)
        rows: List[List[int]] = [[] for _ in range(batch_size)]
        for s, b in zip(mine, _pyramid(batch_size)):
            rows[b].append(s)
        return rows

    def set_schedule(self, orders: Sequence[Sequence[int]]) -> None:
        n = len(self._sequences())
        orders = [[int(s) for s in o] for o in orders]
        B = len(orders)
        if not 1 <= B <= 65535:
            raise ValueError("sast_amd.sampling: the schedule must hold 1 .. 65535 batch rows")
        longest = max(len(o) for o in orders)
        if longest > self.order_capacity:
            raise ValueError(f"sast_amd.sampling: a batch row's schedule holds {longest} sequences, order_capacity is {self.order_capacity}")
        if B * self.order_capacity > 2 ** 31 - 1:
            raise ValueError("sast_amd.sampling: batch rows * order_capacity must stay below 2^31")
        for b, o in enumerate(orders):
            bad = [s for s in o if not 0 <= s < n]
            if bad:
                raise ValueError(f"sast_amd.sampling: batch row {b}'s schedule names sequence {bad[0]}, outside [0, {n})")
        dev = self.status.device
        if self.order is None or self.order.shape[0] != B:
            F.not_capturing("sampling", "set_schedule with a new batch size allocates: call it before graph capture")
            self.order = torch.full((B, self.order_capacity), -1, dtype=torch.int32, device=dev)
            self.order_len = torch.zeros(B, dtype=torch.int32, device=dev)
            self.cursor = torch.zeros(B, 2, dtype=torch.int32, device=dev)
            a = self._args
            a.order, a.order_len, a.cursor = self.order.data_ptr(), self.order_len.data_ptr(), self.cursor.data_ptr()
        if longest:
            host = np.full((B, longest), -1, np.int32)
            for b, o in enumerate(orders):
                host[b, :len(o)] = o
            self.order[:, :longest].copy_(torch.from_numpy(host))
        self.order_len.copy_(torch.tensor([len(o) for o in orders], dtype=torch.int32))
        self.cursor.zero_()
        self._orders = orders

    def _walk(self):
        """per batch row the (sequence, sample) of every step of its schedule"""
        samples = self._sequences()[:, 3]
        if self._orders is None:
            raise RuntimeError("sast_amd.sampling: call set_schedule() before plan() / steps()")
        return [[(s, i) for s in o for i in range(int(samples[s]))] for o in self._orders]

    def steps(self, mode: str = "shortest") -> int:
        if mode not in ("shortest", "longest"):
            raise ValueError("sast_amd.sampling: mode must be 'shortest' (Zipper) or 'longest' (ZipperLongest)")
        n = [len(w) for w in self._walk()]
        return min(n) if mode == "shortest" else max(n)

    def plan(self) -> StreamingPlan:
        walk = self._walk()
        sequences, lw = self._host
        Ls, B, n = self.sequence_length, len(walk), max(len(w) for w in walk)
        K, first, seq = np.zeros(n, np.int64), np.zeros((n, B), bool), np.full((n, B), -1, np.int32)
        for b, w in enumerate(walk):
            for step, (s, i) in enumerate(w):
                r, start, stop, _samples = (int(v) for v in sequences[s])
                lo = start + i * Ls
                K[step] += int(lw[r][lo:min(lo + Ls, stop)].sum())
                first[step, b], seq[step, b] = i == 0, s
        return StreamingPlan(K, first, seq)

    # ---- batches
    def _want(self, B: int):
        Ls, M = self.sequence_length, self.labels.max_labels_per_frame
        i32, u8, i64 = torch.int32, torch.uint8, torch.int64
        return (((B,), i32), ((Ls, B), i32), ((B,), i32), ((B,), i32), ((B,), u8), ((B,), u8), ((Ls, B), i64), ((Ls, B), i64),
                ((Ls, B, M, 7), torch.float32), ((Ls, B), i32), ((Ls, B), u8), ((Ls, B), u8))

    def next(self, out: Optional[Sequence[torch.Tensor]] = None) -> StreamingBatch:
        if out is not None:
            out = tuple(out)
            _need_gpu(*out)               # CPU tensors are refused before anything else is looked at
        if self._args is None:
            raise RuntimeError("sast_amd.sampling: call index() before next()")
        if self.order is None:
            raise RuntimeError("sast_amd.sampling: call set_schedule() before next()")
        dev = self.status.device
        B = self.order.shape[0]
        self._label_elems_guard(B)
        out = F.outputs(StreamingBatch, self._want(B), out, dev, "sampling", "twelve tensors of a StreamingBatch", "the pool's")
        L.check(L.lib().sast_stream_next(C.byref(self.labels._args), C.byref(self._args), B, *(t.data_ptr() for t in out), _stream()),
                "stream_next")
        return out

    def frames(self, batch: StreamingBatch, out_frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._step_frames(batch, out_frames)


class MixedBatch(NamedTuple):
    """what `MixedPool.next` returns (L = sequence_length, M = the labels' max_labels_per_frame, B = Bs + Br: the stream pool's batch
    rows in columns [0, Bs), the random-access samples in columns [Bs, B))"""
    rows: torch.Tensor            # int32 [B]: the pool row (recording) of every column, -1: exhausted, a bad schedule entry or a bad item
    step_rows: torch.Tensor       # int32 [L, B]: the row map of the frames (-1: a padded step or a bad item)
    seq: torch.Tensor             # int32 [B]: as StreamingBatch.seq; -1 for random columns
    sample: torch.Tensor          # int32 [B]: as StreamingBatch.sample; -1 for random columns
    is_first: torch.Tensor        # uint8 [B]: as StreamingBatch.is_first; 1 for random columns (their states are reset every step)
    exhausted: torch.Tensor       # uint8 [B]: as StreamingBatch.exhausted; 0 for random columns
    window_idx: torch.Tensor      # int64 [L, B]
    ends_us: torch.Tensor         # int64 [L, B]
    labels: torch.Tensor          # fp32 [L, B, M, 7]
    counts: torch.Tensor          # int32 [L, B]
    labelled: torch.Tensor        # uint8 [L, B]
    is_padded: torch.Tensor       # uint8 [L, B]: 0 for random columns
    latest: torch.Tensor          # fp32 [Br, M, 7]: RandomAccessBatch.latest
    latest_count: torch.Tensor    # int32 [Br]


class MixedPool:
    """mixed = MixedPool(stream, random)
    bs_str, bs_rnd = MixedPool.batch_sizes(batch_size, w_stream, w_random)
    batch = mixed.next(items, out=None)
    frames = mixed.frames(batch, out_frames=None)
    mixed.prefetch_latest(next_items); latest_labels = mixed.latest_labels()
    mixed.labelled_pairs(step, items_host); mixed.steps(Br); mixed.errors(); mixed.frame_errors()

    The reference's actual training batch of `sampling: 'mixed'`: `set_mixed_sampling_mode_variables_for_train`
    (modules/data/genx.py:116-129) splits the batch size into bs_str streamed and bs_rnd random-access rows, `merge_mixed_batches`
    (modules/utils/detection.py:133-161) concatenates the two loaders' batches along the batch axis, stream rows first, and
    `training_step` runs ONE forward and backward over the result; the random rows are reset every step (their is_first_sample is
    true).  `MixedPool` makes that batch on the device from a `StreamingPool` and a `RandomAccessPool` over the same recordings.

    stream, random: the two pools.  They must share one `LabelStreams`, one sequence_length, one frame geometry and representation,
      and read the same events (`StreamingPool(events=random)`, or `random` itself being the source of `stream`'s source);
      ValueError otherwise.  Neither pool's own calls change: both can still be used alone, on the same cursors and index.
    batch_sizes: host only -- the reference's split, bs_rnd = min(round(batch_size * w_random / (w_stream + w_random)),
      batch_size - 1), bs_str = batch_size - bs_rnd.  ValueError where the reference asserts (batch_size < 2, a weight <= 0) and where
      either part would be 0 (the reference would build a loader with batch size 0).
    next: items int64 [Br] on the device -> `MixedBatch` with Bs = the stream pool's schedule batch.  Columns [0, Bs) are exactly what
      `stream.next()` gives (and the stream cursors move on as they do there), columns [Bs, B) exactly what `random.batch(items)`
      gives; both pools' status words are set as by those calls.  1 launch.
    frames: [L, B, C, H', W'] through ONE row-mapped window search and one histogram pass over step_rows / ends_us: 5 launches for
      the union batch, byte for byte the concatenation of the two pools' frames.  The pool keeps its own error counters
      (`frame_errors()`) and buffers.
    prefetch_latest / latest_labels: zoom-in is drawn on the host from the most recent non-empty label frame of every random sample,
      and its number of draws depends on the label values, so the draw stays the reference's and stays on the host.  The epoch's item
      order is known in advance: `prefetch_latest(next_items)` enqueues `random.latest` for the NEXT step's items (1 launch), copies
      the result into pinned host buffers without blocking and records an event; `latest_labels()` waits on the event of the OLDEST
      look-ahead not handed out yet and returns what `SpatialAugmentor.randomize(latest_labels=)` takes, per row a CPU tensor [k, 7]
      or None.  Two look-aheads may be pending (step n + 1's is enqueued before step n's is read; a third raises), so the one host
      wait per step that remains is on an event recorded a step earlier.  Both stay outside graph capture.  The tensors
      `latest_labels()` returns are views of pinned buffers that the second `prefetch_latest` after it reuses.
    labelled_pairs: host only, no sync -- K of the merged batch: stream.plan().K[step] + random.labelled_pairs(items_host).
    steps: min(stream.steps('shortest'), N // Br) with N the random pool's item count: the epoch stops with the shorter of the two halves.  (How Lightning's
      CombinedLoader ends an epoch over the two loaders is unpinned: pytorch_lightning is not installed.  Any other policy is the
      caller's loop.)
    errors: (stream.errors(), random.errors()).
    After one un-captured call of next and frames with the same Bs and Br nothing is allocated but the outputs and nothing
    synchronises: next + frames (+ joined augmentor + step) are captured in one graph; a replay advances the streams and reads the
    items written into the captured `items` tensor."""

    NEXT_LAUNCHES = 1
    FRAMES_LAUNCHES = 5
    PREFETCH_LAUNCHES = 1

    def __init__(self, stream: StreamingPool, random: RandomAccessPool):
        if not isinstance(stream, StreamingPool) or not isinstance(random, RandomAccessPool):
            raise TypeError("sast_amd.sampling: MixedPool takes a StreamingPool and a RandomAccessPool")
        if stream.labels is not random.labels:
            raise ValueError("sast_amd.sampling: the two pools must share one LabelStreams")
        if stream.sequence_length != random.sequence_length:
            raise ValueError(f"sast_amd.sampling: the pools' sequence_length differ ({stream.sequence_length}, {random.sequence_length})")
        geometry = ("representation", "bins", "height", "width", "count_cutoff", "fastmode", "downsample_by_2", "mode", "value",
                    "window_capacity")
        for name in geometry:
            if getattr(stream, name) != getattr(random, name):
                raise ValueError(f"sast_amd.sampling: the pools' frames differ in {name} ({getattr(stream, name)!r}, "
                                 f"{getattr(random, name)!r})")
        src = stream._events if stream._events is not None else stream
        if src is not random:
            raise ValueError("sast_amd.sampling: the pools must read the same events: build the StreamingPool with events=random")
        self.stream, self.random = stream, random
        self.labels, self.sequence_length, self.num_rows = stream.labels, stream.sequence_length, stream.num_rows
        # the frames driver of the union batch: its own workspace, window bounds and error counters over `random`'s events
        self._driver = _PoolEvents(stream.labels, stream.height, stream.width, stream.sequence_length, stream.bins, stream.count_cutoff,
                                   stream.fastmode, stream.value, stream.downsample_by_2, stream.representation, stream.window_capacity,
                                   events=random, events_name="the random pool")
        # Br -> two slots of (latest [Br, M, 7], latest_count [Br] in pinned host memory, their device sources, an event): the look-ahead
        # of step n + 1 is enqueued while step n's labels are still to be read
        self._pinned = {}
        self._turn = 0
        self._pending = []         # the slots latest_labels() has not handed out yet, oldest first

    # ---- host arithmetic
    @staticmethod
    def batch_sizes(batch_size: int, w_stream, w_random) -> Tuple[int, int]:
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 2:
            raise ValueError("sast_amd.sampling: mixed sampling needs an int batch_size >= 2")
        if not w_random > 0 or not w_stream > 0:
            raise ValueError("sast_amd.sampling: w_stream and w_random must be > 0")
        bs_rnd = min(round(batch_size * w_random / (w_stream + w_random)), batch_size - 1)
        bs_str = batch_size - bs_rnd
        if bs_rnd < 1 or bs_str < 1:
            raise ValueError(f"sast_amd.sampling: batch_size {batch_size} with weights {w_stream} : {w_random} leaves {bs_str} streamed and "
                             f"{bs_rnd} random-access rows; both halves need at least one")
        return bs_str, bs_rnd

    def labelled_pairs(self, step: int, items_host) -> int:
        return int(self.stream.plan().K[step]) + self.random.labelled_pairs(items_host)

    def steps(self, random_batch: int) -> int:
        if isinstance(random_batch, bool) or not isinstance(random_batch, int) or random_batch < 1:
            raise ValueError("sast_amd.sampling: the random-access batch size must be an int >= 1")
        if self.random._host is None:
            raise RuntimeError("sast_amd.sampling: call index() on the random pool before steps()")
        return min(self.stream.steps("shortest"), int(self.random._host[0][-1]) // random_batch)

    def errors(self):
        """(the stream pool's status names, the random pool's (per row, pool-wide) status names) (synchronises)"""
        return self.stream.errors(), self.random.errors()

    def frame_errors(self) -> Tuple[int, int]:
        """(invalid events, windows over capacity) of this pool's frames calls (synchronises)"""
        return self._driver.frame_errors()

    # ---- batches
    def _want(self, Bs: int, Br: int):
        return self.stream._want(Bs + Br) + self.random._want(Br)[-2:]

    def next(self, items: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> MixedBatch:
        sp, rp = self.stream, self.random
        if out is not None:
            out = tuple(out)
            _need_gpu(*out)
        Br = rp._items(items)
        if sp._args is None:
            raise RuntimeError("sast_amd.sampling: call index() on the stream pool before next()")
        if sp.order is None:
            raise RuntimeError("sast_amd.sampling: call set_schedule() on the stream pool before next()")
        dev = items.device
        F.lives_on("the stream pool", sp.status.device, "items", dev, "sampling")
        Bs = sp.order.shape[0]
        sp._label_elems_guard(Bs + Br)
        out = F.outputs(MixedBatch, self._want(Bs, Br), out, dev, "sampling", "fourteen tensors of a MixedBatch", "the pool's")
        L.check(L.lib().sast_mixed_next(C.byref(self.labels._args), C.byref(sp._args), C.byref(rp._args), Bs, items.data_ptr(), Br,
                                        *(t.data_ptr() for t in out), _stream()), "mixed_next")
        return out

    def frames(self, batch: MixedBatch, out_frames: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._driver._step_frames(batch, out_frames)

    # ---- the zoom-in look-ahead
    def prefetch_latest(self, next_items: torch.Tensor) -> None:
        Br = self.random._items(next_items)
        F.not_capturing("sampling", "prefetch_latest copies to the host: keep it outside graph capture")
        if len(self._pending) >= 2:
            raise RuntimeError("sast_amd.sampling: two look-aheads are pending: call latest_labels() before the next prefetch_latest()")
        M = self.labels.max_labels_per_frame
        if Br not in self._pinned:
            dev = next_items.device
            self._pinned[Br] = [(torch.empty(Br, M, 7, dtype=torch.float32).pin_memory(), torch.empty(Br, dtype=torch.int32).pin_memory(),
                                 RandomAccessLatest(torch.empty(Br, M, 7, dtype=torch.float32, device=dev),
                                                    torch.empty(Br, dtype=torch.int32, device=dev)), torch.cuda.Event()) for _ in range(2)]
        self._turn ^= 1
        host, host_count, staged, event = slot = self._pinned[Br][self._turn]
        self.random.latest(next_items, out=staged)
        host.copy_(staged.latest, non_blocking=True)
        host_count.copy_(staged.latest_count, non_blocking=True)
        event.record()
        self._pending.append(slot)

    def latest_labels(self) -> List[Optional[torch.Tensor]]:
        if not self._pending:
            raise RuntimeError("sast_amd.sampling: call prefetch_latest() before latest_labels()")
        F.not_capturing("sampling", "latest_labels waits for a host copy: keep it outside graph capture")
        host, host_count, _staged, event = self._pending.pop(0)
        event.synchronize()
        return [host[b, :k] if k else None for b, k in enumerate(host_count.tolist())]
