"""Raw events (x, y, p, t) -> stacked-histogram or mixed-density frames on the GPU (csrc/k_events.hip).

The reference builds the detector's input offline on the CPU: StackedHistogram.construct (data/utils/representations.py:37-121) once per
window of scripts/genx/preprocess_dataset.py:476-530, on timestamps its reader forced non-decreasing (:159-168) with negative polarities
clipped to 0 (:177), downsampled by 2 with nearest-exact interpolation for Gen4 (:463-473).  Both classes here give the same uint8 frames,
bit for bit, from device tensors:

- `StackedHistogram`: the reference's class and `construct(x, y, pol, time)` signature (one window: the whole arrays, time assumed sorted).
- `EventFrames`: the streaming front end.  One event buffer, a tensor of window ends, duration or count windows, the reader's time
  correction with its carry kept on the device, optional downsampling by 2 -> uint8 [B, 2*bins, H', W'], the input of `RNNDetector` /
  `YoloXDetector`.  Every per-frame value stays on the device, so a call can be captured in a graph and replayed on new events written
  into the same buffers.

The reference's second representation, MixedDensityEventStack (representations.py:130-218: signed int8 frames of `bins` channels, events
binned by the logarithm of their age and accumulated over the bins), is `MixedDensityEventStack` here, and
`representation="mixed_density"` of `EventFrames` / `EventStreams`: the same windows, carries and error counters, int8 frames.

`EventQueue` keeps the events that later windows still need on the device, so a host pushes chunks cut at arbitrary points (columns,
Prophesee's packed Event2D records, or the raw EVT 3.0 / EVT 2.0 / EVT 2.1 words of a sensor) and gets the frames `EventStreams`
gives for the whole recording.  `Evt3Decoder` (csrc/k_evt3.hip) and `Evt2Decoder` (csrc/k_evt2.hip) are the stateful decodes of those
words alone (one driver, csrc/evt_dec.cuh, and a small policy per format; here `_EventDecoder` and two subclasses); `raw_header`
(host only) reads the format, the geometry and the end of a .raw file's ASCII header.  `Evt3Encoder` (csrc/k_evt3_enc.hip) and `Evt2Encoder` (csrc/k_evt2_enc.hip) are the way back, columns or Event2D records -> EVT 3.0 / 2.0 / 2.1
words, and `evt3_raw_header` / `evt2_raw_header` (host only) write the header such a file starts with.  `EventFilter`
(csrc/k_evfilter.hip) is the event-level noise filtering between decode and accumulate: the background-activity and the
spatio-temporal-contrast filter, alone or as `EventQueue(filter=...)` in front of every push.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _frontend as F
from . import _lib as L
from .functional import _need_gpu, _stream


def _columns(x, y, pol, time):
    _need_gpu(x, y, pol, time)
    cols = []
    for t, name in ((x, "x"), (y, "y"), (pol, "pol"), (time, "time")):
        if t.dim() != 1:
            raise ValueError(f"sast_amd.events: {name} must be 1-D, got shape {tuple(t.shape)}")
        cols.append(t.contiguous())
    if not x.numel() == y.numel() == pol.numel() == time.numel():
        raise ValueError("sast_amd.events: x, y, pol and time must hold the same number of events")
    F.same_device("events", "x, y, pol and time", *cols)
    codes = [F.dtype_code(cols[0], "x", "events"), F.dtype_code(cols[1], "y", "events"), F.dtype_code(cols[2], "pol", "events"),
             F.dtype_code(cols[3], "time", "events", (torch.int64, torch.int32))]
    return cols, codes


def _cutoff(count_cutoff: Optional[int]) -> int:
    # representations.py:51-56: None means 255, larger values are capped at 255
    if count_cutoff is None:
        return 255
    if int(count_cutoff) < 1:
        raise ValueError("sast_amd.events: count_cutoff must be >= 1 (or None)")
    return min(int(count_cutoff), 255)


def _md_cutoff(count_cutoff: Optional[int]) -> Optional[int]:
    # representations.py:139-142: None, or an int in 0 .. 127
    if count_cutoff is None:
        return None
    if isinstance(count_cutoff, bool) or not isinstance(count_cutoff, int) or not 0 <= count_cutoff <= 127:
        raise ValueError("sast_amd.events: the mixed-density count_cutoff must be an int in 0 .. 127 (or None)")
    return count_cutoff


REPRESENTATIONS = ("stacked_histogram", "mixed_density")


class _Frames:
    """geometry + the device workspace of sast_event_frames / sast_mdstack_frames (zero when created, left zero by every call)"""

    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int], fastmode: bool, downsample_by_2: bool,
                 representation: str = "stacked_histogram"):
        if int(bins) < 1 or int(height) < 1 or int(width) < 1:
            raise ValueError("sast_amd.events: bins, height and width must be >= 1")
        if representation not in REPRESENTATIONS:
            raise ValueError(f"sast_amd.events: representation must be one of {REPRESENTATIONS}, got {representation!r}")
        self.representation = representation
        self.mixed_density = representation == "mixed_density"
        self.bins, self.height, self.width = int(bins), int(height), int(width)
        if self.mixed_density:
            if fastmode is not True:
                raise ValueError("sast_amd.events: fastmode does not apply to the mixed-density representation")
            self.count_cutoff = _md_cutoff(count_cutoff)
        else:
            self.count_cutoff = _cutoff(count_cutoff)
        self.frame_dtype = torch.int8 if self.mixed_density else torch.uint8
        self.fastmode = bool(fastmode)
        self.downsample_by_2 = bool(downsample_by_2)
        self.out_hw = (self.height // 2, self.width // 2) if self.downsample_by_2 else (self.height, self.width)
        self._ws = {}

    def get_shape(self) -> Tuple[int, int, int]:
        return (self.bins if self.mixed_density else 2 * self.bins), self.out_hw[0], self.out_hw[1]

    def ws_bytes(self, B: int, window_capacity: int) -> int:
        query = L.lib().sast_mdstack_frames_ws_bytes if self.mixed_density else L.lib().sast_event_frames_ws_bytes
        n = int(query(B, self.bins, self.height, self.width, int(self.downsample_by_2), int(window_capacity)))
        if n == 0:
            raise ValueError(f"sast_amd.events: unsupported frame geometry (B={B}, bins={self.bins}, {self.height}x{self.width}, "
                             f"window capacity {window_capacity}); " + ("bins <= 512" if self.mixed_density else "2*bins <= 640"))
        return n

    def workspace(self, device, B: int, window_capacity: int) -> torch.Tensor:
        # the record area comes last in the layout: a workspace made for more events per window serves fewer as well
        need = self.ws_bytes(B, window_capacity)
        key = (device, B)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            F.not_capturing("events")
            self._ws.clear()
            ws = self._ws[key] = torch.zeros(need, dtype=torch.uint8, device=device)
        return ws

    def launch(self, cols, codes, capacity: int, bounds: torch.Tensor, out: torch.Tensor, err: torch.Tensor, window_capacity: int,
               clip_negative_polarity: bool):
        B = bounds.shape[0]
        ws = self.workspace(out.device, B, window_capacity)
        a = L.SastMdStackArgs() if self.mixed_density else L.SastEventArgs()
        x, y, p, t = cols
        # an empty column has no storage: any valid device pointer will do, the kernels read no event
        a.x, a.y, a.p, a.t = (c.data_ptr() or out.data_ptr() for c in (x, y, p, t))
        a.bounds, a.out, a.err, a.ws = bounds.data_ptr(), out.data_ptr(), err.data_ptr(), ws.data_ptr()
        a.capacity, a.window_capacity = int(capacity), int(window_capacity)
        a.x_dtype, a.y_dtype, a.p_dtype, a.t_dtype = codes
        a.B, a.bins, a.height, a.width = B, self.bins, self.height, self.width
        a.downsample_by_2, a.clip_negative_polarity = int(self.downsample_by_2), int(clip_negative_polarity)
        if self.mixed_density:
            a.count_cutoff = -1 if self.count_cutoff is None else self.count_cutoff
            L.check(L.lib().sast_mdstack_frames(C.byref(a), _stream()), "mdstack_frames")
            return
        a.count_cutoff, a.fastmode = self.count_cutoff, int(self.fastmode)
        L.check(L.lib().sast_event_frames(C.byref(a), _stream()), "event_frames")

    def construct(self, x: torch.Tensor, y: torch.Tensor, pol: torch.Tensor, time: torch.Tensor, check: bool = True) -> torch.Tensor:
        """one window, the whole arrays (time sorted) -> frame_dtype [C, height, width]: the reference classes' `construct`"""
        cols, codes = _columns(x, y, pol, time)
        dev = cols[0].device
        n = cols[0].numel()
        bounds = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
        err = torch.zeros(2, dtype=torch.int32, device=dev)
        out = torch.empty((1,) + self.get_shape(), dtype=self.frame_dtype, device=dev)
        self.launch(cols, codes, n, bounds, out, err, max(n, 1), clip_negative_polarity=False)
        if check:
            _raise_on_errors(err)
        return out[0]


def _raise_on_errors(err: torch.Tensor):
    bad, over = (int(v) for v in err.tolist())
    if bad:
        raise ValueError(f"sast_amd.events: {bad} invalid events (x or y outside the sensor, or a polarity outside 0..1); they were skipped")
    if over:
        raise ValueError(f"sast_amd.events: {over} windows hold more events than window_capacity; they were left empty")


class StackedHistogram(_Frames):
    """representations.py:37-121 on device tensors: `construct(x, y, pol, time)` -> uint8 [2*bins, height, width].

    x, y, pol: int64 / int32 / int16; time: int64 / int32, sorted (the reference's assumption: the first and last timestamps set the
    time bins).  Invalid events (x or y outside the sensor, pol outside 0..1, a time before time[0]), which the reference rejects with an
    assertion or an index error, are skipped and counted; with check=True (the default) construct synchronises and raises ValueError."""

    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int] = None, fastmode: bool = True):
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2=False)
        self.channels = 2

    @staticmethod
    def get_torch_dtype() -> torch.dtype:
        return torch.uint8

    @property
    def dtype(self) -> torch.dtype:
        return torch.uint8


class MixedDensityEventStack(_Frames):
    """representations.py:130-218 on device tensors: `construct(x, y, pol, time)` -> int8 [bins, height, width].

    Events are binned by the logarithm of their age: with t_norm = (t - time[0]) / max(time[-1] - time[0], 1) in fp32, clamped to
    [1e-6, 1 - 1e-6], bin = max(bins + floor(log2(t_norm)), 0) (the last bin holds the older half of the window, the one before it the
    quarter before that, ...); each event adds 2*pol - 1, channel i is the sum of channels 0..i, wrapped to int8, then clamped to
    [-count_cutoff, count_cutoff] (count_cutoff: an int in 0 .. 127, or None for no clamp).  The bin is read from the fp32 exponent, which
    equals the reference's floor(bins - log(t_norm) / log(1/2)) as long as neighbouring integer times stay distinguishable in fp32 near a
    bin boundary: window spans up to about 2 s.  Column dtypes, invalid events and `check` as in `StackedHistogram`."""

    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int] = None):
        super().__init__(bins, height, width, count_cutoff, True, downsample_by_2=False, representation="mixed_density")

    @staticmethod
    def get_torch_dtype() -> torch.dtype:
        return torch.int8

    @property
    def dtype(self) -> torch.dtype:
        return torch.int8


class _Windowed(_Frames):
    """what `EventFrames` and `EventStreams` share: the window rule (duration or count), the time-correction carry `t_last`, the error
    counters `err`, and the buffers kept between calls (among them one `bounds` tensor per number of windows asked for).  Those are
    allocated by ordinary calls only: one un-captured warm-up call with the same sizes is needed before a call can be captured in a
    graph."""

    _module = "events"         # the module named in front of this object's messages

    def __init__(self, bins: int, height: int, width: int, count_cutoff: Optional[int], fastmode: bool, downsample_by_2: bool,
                 representation: str, duration_us: Optional[int], num_events: Optional[int], correct_time: bool,
                 window_capacity: Optional[int]):
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2, representation)
        if (duration_us is None) == (num_events is None):
            raise ValueError("sast_amd.events: give exactly one of duration_us and num_events")
        if (duration_us if duration_us is not None else num_events) < (0 if duration_us is not None else 1):
            raise ValueError("sast_amd.events: duration_us must be >= 0, num_events >= 1")
        self.mode = L.EVENT_WINDOW_DURATION if duration_us is not None else L.EVENT_WINDOW_COUNT
        self.value = int(duration_us if duration_us is not None else num_events)
        self.correct_time = bool(correct_time)
        self.window_capacity = None if window_capacity is None else int(window_capacity)
        self.t_last: Optional[torch.Tensor] = None
        self.err: Optional[torch.Tensor] = None
        self.last_bounds: Optional[torch.Tensor] = None
        self._state = {}

    def _carry(self, dev, shape):
        if self.t_last is None or self.t_last.device != dev:
            self.t_last = torch.zeros(shape, dtype=torch.int64, device=dev)
            self.err = torch.zeros(2, dtype=torch.int32, device=dev)

    def _bounds(self, windows: int, dev, hint: str = "number of windows") -> torch.Tensor:
        """the int64 [windows, 2] tensor the window search writes, kept per window count so that a captured call finds it again"""
        kept = self._state.setdefault("bounds", {})
        if windows not in kept:
            F.not_capturing(self._module, f"one un-captured warm-up call with the same {hint} is needed before graph capture")
            kept[windows] = torch.empty(windows, 2, dtype=torch.int64, device=dev)
        return kept[windows]

    def _frames_shape(self, ends_us: torch.Tensor, S: int, cap: int) -> Tuple[int, int, tuple]:
        """ends_us int64 [S] or [T, S] -> (T, the window capacity of a call on rows of `cap` events, the frames' shape)"""
        T = F.window_ends(ends_us, S, "events")
        wcap = self.window_capacity if self.window_capacity is not None else max(cap, 1)
        self.ws_bytes(T * S, wcap)              # ValueError for more windows than the frame kernels take
        return T, wcap, tuple(ends_us.shape) + self.get_shape()

    def errors(self) -> Tuple[int, int]:
        """(invalid events, windows over capacity) since the last reset() (synchronises)"""
        return F.counters(self.err, 2)


class EventFrames(_Windowed):
    """Batched stacked-histogram frames from one event buffer (the windowing of preprocess_dataset.py:507-530).

    frames = ef(x, y, p, t, ends_us, n=None) -> uint8 [B, 2*bins, H', W'] (H' = height // 2, W' = width // 2 with downsample_by_2).
      x, y, p: int64 / int32 / int16;  t: int64 / int32;  ends_us: int64 [B] window end times (microseconds);
      n: the number of valid events at the head of the buffers, a device int64 tensor of one element (default: the buffers' length).
    Windows: duration_us=D -> events with ends_us[b] - D <= t <= ends_us[b];  num_events=N -> the last N events with t <= ends_us[b].
    correct_time (default True): the reader's correction first -- t[i] = max(t[i], running max) -- with the
      running maximum carried across calls in `t_last` (a device tensor; `reset()` sets it back to 0 for a new recording).  The buffer
      passed in is not modified: the corrected timestamps go to an internal int64 buffer.  correct_time=False takes t as it is (int64,
      sorted) and leaves the carry alone.  Negative polarities are clipped to 0, as the reader does.  Each call continues the
      recording: feeding the same events again without reset() raises every timestamp to the carry (the last call's maximum).
    window_capacity: kept events one window may hold (default: the buffers' length); a window over it is left zero and reported.
    check=False (the default) never synchronises, so a call can be captured in a graph; errors accumulate in `err` (int32 [2]:
      invalid events -- each counted once, among the events the windows hold --, windows over capacity) until `reset()`.  check=True clears them, synchronises after the call and raises
      ValueError if the call met any.
    representation="mixed_density": the frames are the mixed-density event stack (`MixedDensityEventStack`) of every window instead,
      int8 [B, bins, H', W']; count_cutoff is then an int in 0 .. 127 or None, and fastmode does not apply.  Everything else is unchanged."""

    def __init__(self, height: int, width: int, bins: int = 10, count_cutoff: Optional[int] = 10, fastmode: bool = True,
                 duration_us: Optional[int] = None, num_events: Optional[int] = None, downsample_by_2: bool = False,
                 correct_time: bool = True, window_capacity: Optional[int] = None, representation: str = "stacked_histogram"):
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2, representation, duration_us, num_events,
                         correct_time, window_capacity)

    def _buffers(self, dev, capacity: int):
        st = self._state.get("cap")
        if st is None or st[0] != dev or st[1] < capacity:
            F.not_capturing("events")
            self._state = {"cap": (dev, capacity), "t": torch.empty(max(capacity, 1), dtype=torch.int64, device=dev),
                           "scan": torch.empty(L.EVENT_SCAN_BLOCKS + 1, dtype=torch.int64, device=dev)}
        self._carry(dev, ())
        return self._state

    def reset(self):
        """a new recording: the time-correction carry back to 0, the error counters cleared"""
        F.reset_rows((self.t_last,), self.err, None, 1, "events")

    def __call__(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, ends_us: torch.Tensor,
                 n: Optional[torch.Tensor] = None, check: bool = False) -> torch.Tensor:
        cols, codes = _columns(x, y, p, t)
        _need_gpu(ends_us, n)
        if ends_us.dim() != 1 or ends_us.dtype != torch.int64 or ends_us.numel() < 1:
            raise ValueError("sast_amd.events: ends_us must be a 1-D int64 tensor of at least one window end")
        dev = cols[0].device
        cap = cols[0].numel()
        st = self._buffers(dev, cap)
        if n is None:
            n = st.get("n")
            if n is None or int(st["n_val"]) != cap:
                F.not_capturing("events", "pass n (a device tensor) when capturing, or warm up with the same buffer length")
                n = st["n"] = torch.full((1,), cap, dtype=torch.int64, device=dev)
                st["n_val"] = cap
        elif n.dtype != torch.int64 or n.numel() != 1:
            raise ValueError("sast_amd.events: n must be a one-element int64 device tensor")
        if check:
            self.err.zero_()
        B = ends_us.numel()
        wcap = self.window_capacity if self.window_capacity is not None else max(cap, 1)
        if self.correct_time:
            tc = st["t"]
            L.check(L.lib().sast_event_correct_time(cols[3].data_ptr() or tc.data_ptr(), codes[3], n.data_ptr(), cap, tc.data_ptr(),
                                                    self.t_last.data_ptr(), st["scan"].data_ptr(), _stream()), "event_correct_time")
            cols = cols[:3] + [tc[:max(cap, 1)]]
            codes = codes[:3] + [L.DT_I64]
        elif cols[3].dtype != torch.int64:
            raise TypeError("sast_amd.events: correct_time=False needs int64 timestamps")
        bounds = torch.empty(B, 2, dtype=torch.int64, device=dev)
        L.check(L.lib().sast_event_window_bounds(cols[3].data_ptr() or st["t"].data_ptr(), n.data_ptr(), cap, ends_us.contiguous().data_ptr(),
                                                 B, self.mode, self.value, bounds.data_ptr(), _stream()), "event_window_bounds")
        out = torch.empty((B,) + self.get_shape(), dtype=self.frame_dtype, device=dev)
        self.launch(cols, codes, cap, bounds, out, self.err, wcap, clip_negative_polarity=True)
        self.last_bounds = bounds
        if check:
            _raise_on_errors(self.err)
        return out


class EventStreams(_Windowed):
    """`EventFrames` for S recordings side by side: frames for every recording, and for T steps of each, in one call.

    frames = es(x, y, p, t, counts, ends_us, reset=None, check=False, out=None)
      x, y, p, t: contiguous [S, cap] device tensors (dtypes as in `EventFrames`), row s one recording with its events at the head of the row;
      counts: int64 [S], the valid events of each row (what lies past them is never read);
      ends_us: int64 [S] -> uint8 [S, 2*bins, H', W'], or int64 [T, S] -> uint8 [T, S, 2*bins, H', W'] (the layout `SpatialAugmentor` and
        `TrainStep` take); ends_us[k, s] is a window end on recording s's own clock;
      reset: uint8 / bool [S] device tensor, non-zero for the rows that start a new recording with this call: their time-correction carry
        starts at 0 (the device-side counterpart of `reset(streams=...)`, for a captured call);
      out: the uint8 tensor to write (default: a new one from the caching allocator, as `EventFrames` returns).
    Every row has its own carry (`t_last`, int64 [S]) and its own windows: the running maximum of the time correction never crosses
    from one row into the next, a count window stops at the start of its row.  One call is 7 library launches whatever S and T are
    (2 time correction, 1 window search, 4 histogram; 5 with correct_time=False).  After one un-captured warm-up call with the same
    shapes nothing is allocated but `out`, and nothing synchronises: the `bounds` tensor (`last_bounds`, int64 [T*S, 2], indices into
    the flattened [S*cap] buffer) is kept in the object, so a call can be captured in a graph and replayed on new events, counts, ends and reset
    flags written into the same tensors.
    window_capacity: kept events one window may hold (default: cap, one row); the workspace holds T*S*window_capacity records.
    `err`, `errors()`, check=True: as in `EventFrames`; the counters are global to the call, not per row.
    representation="mixed_density": as in `EventFrames`, int8 [S, bins, H', W'] / [T, S, bins, H', W'] frames (and an int8 `out`), in the
      same 7 launches."""

    def __init__(self, num_streams: int, height: int, width: int, bins: int = 10, count_cutoff: Optional[int] = 10, fastmode: bool = True,
                 duration_us: Optional[int] = None, num_events: Optional[int] = None, downsample_by_2: bool = False,
                 correct_time: bool = True, window_capacity: Optional[int] = None, representation: str = "stacked_histogram"):
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2, representation, duration_us, num_events,
                         correct_time, window_capacity)
        self.num_streams = F.stream_count(num_streams, "events")

    def _buffers(self, dev, cap: int):
        S = self.num_streams
        st = self._state
        if st.get("cap") is None or st["cap"][0] != dev or st["cap"][1] < cap:
            F.not_capturing("events")
            st = self._state = {"cap": (dev, cap), "t": torch.empty(max(S * cap, 1), dtype=torch.int64, device=dev),
                                "scan": torch.empty(int(L.lib().sast_evstreams_ws_count(S)), dtype=torch.int64, device=dev)}
        self._carry(dev, (S,))
        return st

    def reset(self, streams=None):
        """new recordings, from the host: the time-correction carry of `streams` (default: all of them) back to 0; with streams=None the
        error counters are cleared as well"""
        F.reset_rows((self.t_last,), self.err, streams, self.num_streams, "events")

    def __call__(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor, ends_us: torch.Tensor,
                 reset: Optional[torch.Tensor] = None, check: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        S = self.num_streams
        codes = F.event_columns(x, y, p, t, S, "events")
        if not self.correct_time and t.dtype != torch.int64:
            raise TypeError("sast_amd.events: correct_time=False needs int64 timestamps")
        F.counts_reset(counts, reset, S, "events")
        dev = x.device
        cap = x.shape[1]
        if S * cap > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * capacity must be below 2^31")
        T, wcap, shape = self._frames_shape(ends_us, S, cap)
        _need_gpu(x, y, p, t, counts, ends_us, reset, out)
        F.same_device("events", "x, y, p, t, counts, ends_us and reset", x, y, p, t, counts, ends_us, reset)
        out = F.frames_out(out, shape, self.frame_dtype, dev, "events", "out", "the events'")
        st = self._buffers(dev, cap)
        bounds = self._bounds(T * S, dev)
        if check:
            self.err.zero_()
        lib = L.lib()
        tc = st["t"]
        if self.correct_time:
            L.check(lib.sast_evstreams_correct_time(t.data_ptr() or tc.data_ptr(), codes[3], counts.data_ptr(), S, cap, tc.data_ptr(),
                                                    self.t_last.data_ptr(), None if reset is None else reset.data_ptr(),
                                                    st["scan"].data_ptr(), _stream()), "evstreams_correct_time")
            tcol, codes = tc, codes[:3] + [L.DT_I64]
        else:
            tcol = t
        L.check(lib.sast_evstreams_window_bounds(tcol.data_ptr() or tc.data_ptr(), counts.data_ptr(), S, cap, ends_us.data_ptr(), T,
                                                 self.mode, self.value, bounds.data_ptr(), _stream()), "evstreams_window_bounds")
        self.launch([x, y, p, tcol], codes, S * cap, bounds, out, self.err, wcap, clip_negative_polarity=True)
        self.last_bounds = bounds
        if check:
            _raise_on_errors(self.err)
        return out


_WORD_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)


class _EventDecoder:
    """what `Evt3Decoder` and `Evt2Decoder` share (the device side shares csrc/evt_dec.cuh): the buffers, the argument rules, the
    counters and the call.  A subclass names its entry points, the width of its state, its word dtypes with the words of their
    message and `fanout`, the events one word can give."""

    DECODE_LAUNCHES = 2
    _STATE_WORDS = _WS_BYTES = _DECODE = _dtypes = _what = fanout = None
    _EXTRA = ()                                                      # the arguments between S and reset: EVT 2's version code

    def __init__(self, num_streams: int, max_events: Optional[int] = None):
        self.num_streams = F.stream_count(num_streams, "events")
        if max_events is not None and int(max_events) < 1:
            raise ValueError("sast_amd.events: max_events must be >= 1 (or None)")
        self.max_events = None if max_events is None else int(max_events)
        if self.max_events is not None and self.num_streams * self.max_events > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * max_events must be below 2^31")
        self.state = self.err = self.counts = self.x = self.y = self.p = self.t = self._ws = None

    def _room(self, chunk_words: int) -> int:
        """the staging columns one row needs for a chunk of chunk_words"""
        return self.max_events if self.max_events is not None else max(self.fanout * chunk_words, 1)

    def _buffers(self, dev, chunk_words: int):
        S = self.num_streams
        if self.state is None:
            F.not_capturing("events")
            self.state = torch.zeros(S, getattr(L, self._STATE_WORDS), dtype=torch.int64, device=dev)
            self.err = torch.zeros(3, dtype=torch.int32, device=dev)
            self.counts = torch.zeros(S, dtype=torch.int64, device=dev)
            self._ws = torch.zeros(int(getattr(L.lib(), self._WS_BYTES)(S)), dtype=torch.uint8, device=dev)
        F.lives_on("the decoder's state", self.state.device, "the call's tensors", dev, "events")
        need = self._room(chunk_words)
        if self.x is None or self.x.shape[1] < need:
            F.not_capturing("events")
            if S * need > 2 ** 31 - 1:
                raise ValueError("sast_amd.events: num_streams * max_events must be below 2^31")
            self.x, self.y, self.p = (torch.zeros(S, need, dtype=torch.int16, device=dev) for _ in range(3))
            self.t = torch.zeros(S, need, dtype=torch.int64, device=dev)

    def errors(self) -> Tuple[int, int, int]:
        """(events before the first TIME_HIGH, unknown words, events dropped for lack of staging) since the last reset() (synchronises)"""
        return F.counters(self.err, 3)

    def reset(self, streams=None):
        """new recordings, from the host: the decoder state of `streams` (default: all of them) back to zero; with streams=None the
        counters are cleared as well"""
        F.reset_rows((self.state,), self.err, streams, self.num_streams, "events")

    def __call__(self, words: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None):
        S = self.num_streams
        F.tensor_arg(words, "words", "events", self._dtypes, (("num_streams", S), "chunk words"), self._what, empty_ok=True,
                     dtype_error=TypeError)
        F.counts_reset(counts, reset, S, "events")
        chunk_words = words.shape[1]
        if S * chunk_words > 2 ** 31 - 1 or self.fanout * chunk_words > 2 ** 31 - 1:
            raise ValueError(f"sast_amd.events: num_streams * chunk words and {self.fanout} * chunk words must be below 2^31")
        _need_gpu(words, counts, reset)
        F.same_device("events", "words, counts and reset", words, counts, reset)
        self._buffers(counts.device, chunk_words)
        # an empty chunk has no storage: any valid device pointer will do, the kernels read no word
        L.check(getattr(L.lib(), self._DECODE)(words.data_ptr() or self.t.data_ptr(), counts.data_ptr(), chunk_words, S, *self._EXTRA,
                                               None if reset is None else reset.data_ptr(), self.state.data_ptr(), self._ws.data_ptr(),
                                               self.x.data_ptr(), self.y.data_ptr(), self.p.data_ptr(), self.t.data_ptr(),
                                               self.x.shape[1], self.counts.data_ptr(), self.err.data_ptr(), _stream()),
                self._DECODE[len("sast_"):])
        return self.x, self.y, self.p, self.t, self.counts


class Evt3Decoder(_EventDecoder):
    """Prophesee EVT 3.0 sensor words -> event columns on the device (csrc/k_evt3.hip; the format table and the decode rule are in
    include/sast_hip.h and INTEGRATION.md §3b; parity with the Metavision SDK's decoder is unpinned, the SDK is not a dependency).

    dec = Evt3Decoder(num_streams, max_events=None)
    x, y, p, t, n = dec(words, counts, reset=None)
      words: int16 / uint16 [S, chunk_words], the raw little-endian 16-bit words of S sensors side by side, cut anywhere (`raw_header`
        finds the end of a .raw file's ASCII header); counts: int64 [S], the words at the head of each row; reset: uint8 / bool [S], non-zero for
        the rows whose decoder state (row, vector base, time) is zeroed before this chunk: a new recording.
      -> x, y, p int16 [S, max_events], t int64 [S, max_events] (microseconds, wraps of the 24-bit sensor clock unrolled), n int64 [S]
        the events at the head of each row: what `EventQueue.push` / `EventStreams` take.  The tensors are the decoder's staging
        columns: the next call overwrites them.
    The state after a chunk is the state before the next one, per row: a stream decoded in chunks cut at any word gives the events of
    the stream decoded whole.  max_events: the events one row's chunk may give (default 12 * chunk_words, which can never drop one);
    of a row with more, the first max_events are kept and the rest counted.  `errors()` -> (events before the first TIME_HIGH, unknown
    words, events dropped because the staging was full), accumulated until `reset()`; `reset(streams=None)` zeroes the decoder state of
    the rows (default: all, and the counters).  `state` is int64 [S, 8]: y, base_x, vpol, low, high, wraps, have_high, 0.
    The state and the staging columns are allocated by the first un-captured call, never during capture; afterwards nothing is
    allocated and nothing synchronises.  One call is 2 launches whatever S and the sizes are."""

    _STATE_WORDS, _WS_BYTES, _DECODE = "EVT3_STATE_WORDS", "sast_evt3_ws_bytes", "sast_evt3_decode"
    _dtypes, _what, fanout = _WORD_DTYPES, "(one EVT 3.0 word each)", 12


class _EventEncoder:
    """what `Evt3Encoder` and `Evt2Encoder` share (the device side shares csrc/evt_enc.cuh): the buffers, the argument rules, the
    counters and the call.  A subclass names its entry points, its word dtype and the room a chunk needs by default."""

    ENCODE_LAUNCHES = 2
    _STATE_WORDS = _WS_BYTES = _ENCODE = _ENCODE_DAT = _word_dtype = None
    _EXTRA = ()                                                      # the arguments between S and reset: EVT 2's version code

    def __init__(self, num_streams: int, max_words: Optional[int] = None):
        self.num_streams = F.stream_count(num_streams, "events")
        if max_words is not None and int(max_words) < 1:
            raise ValueError("sast_amd.events: max_words must be >= 1 (or None)")
        self.max_words = None if max_words is None else int(max_words)
        if self.max_words is not None and self.num_streams * self.max_words > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * max_words must be below 2^31")
        self.state = self.err = self.n_words = self.words = self._ws = None

    def _room(self, chunk_events: int) -> int:
        raise NotImplementedError

    def _buffers(self, dev, chunk_events: int):
        S = self.num_streams
        if self.state is None:
            F.not_capturing("events")
            self.state = torch.zeros(S, getattr(L, self._STATE_WORDS), dtype=torch.int64, device=dev)
            self.err = torch.zeros(4, dtype=torch.int32, device=dev)
            self.n_words = torch.zeros(S, dtype=torch.int64, device=dev)
            self._ws = torch.zeros(int(getattr(L.lib(), self._WS_BYTES)(S)), dtype=torch.uint8, device=dev)
        F.lives_on("the encoder's state", self.state.device, "the call's tensors", dev, "events")
        need = self.max_words if self.max_words is not None else self._room(chunk_events)
        if self.words is None or self.words.shape[1] < need:
            F.not_capturing("events")
            if S * need > 2 ** 31 - 1:
                raise ValueError("sast_amd.events: num_streams * max_words must be below 2^31")
            self.words = torch.zeros(S, need, dtype=self._word_dtype, device=dev)

    def errors(self) -> Tuple[int, int, int, int]:
        """(times raised to the running maximum, events with x, y or p clamped, rows refused for lack of room, 0) since the last
        reset() (synchronises)"""
        return F.counters(self.err, 4)

    def reset(self, streams=None):
        """new recordings, from the host: the encoder state of `streams` (default: all of them) back to zero; with streams=None the
        counters are cleared as well"""
        F.reset_rows((self.state,), self.err, streams, self.num_streams, "events")

    def _encode(self, entry, head, chunk_events, counts, reset, tensors):
        S = self.num_streams
        F.counts_reset(counts, reset, S, "events")
        if S * chunk_events > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * chunk events must be below 2^31")
        _need_gpu(*tensors, counts, reset)
        F.same_device("events", "the chunk, counts and reset", *tensors, counts, reset)
        self._buffers(counts.device, chunk_events)
        # an empty chunk has no storage: any valid device pointer will do, the kernels read no event
        head = [h or counts.data_ptr() for h in head[:len(tensors)]] + list(head[len(tensors):])
        L.check(getattr(L.lib(), entry)(*head, counts.data_ptr(), chunk_events, S, *self._EXTRA,
                                        None if reset is None else reset.data_ptr(), self.state.data_ptr(), self._ws.data_ptr(),
                                        self.words.data_ptr(), self.words.shape[1], self.n_words.data_ptr(), self.err.data_ptr(),
                                        _stream()), entry[len("sast_"):])
        return self.words, self.n_words

    def __call__(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor,
                 reset: Optional[torch.Tensor] = None):
        codes = F.event_columns(x, y, p, t, self.num_streams, "events", cap_name="chunk events")
        return self._encode(self._ENCODE, [c.data_ptr() for c in (x, y, p, t)] + list(codes), x.shape[1], counts, reset, [x, y, p, t])

    def encode_dat(self, records: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None):
        F.tensor_arg(records, "records", "events", (torch.int32,), (("num_streams", self.num_streams), "chunk events", 2),
                     "(two words per Event2D record)", empty_ok=True, dtype_error=TypeError)
        return self._encode(self._ENCODE_DAT, [records.data_ptr()], records.shape[1], counts, reset, [records])


class Evt3Encoder(_EventEncoder):
    """Event columns or packed Event2D records -> Prophesee EVT 3.0 sensor words on the device (csrc/k_evt3_enc.hip; the word table and
    the canonical rule are in include/sast_hip.h and INTEGRATION.md §3b; parity with the Metavision SDK's encoder is unpinned, the SDK
    is not a dependency: what is pinned is the sequential model of tests/evt3_encoder_model.py, and that `Evt3Decoder` gives the events
    back).

    enc = Evt3Encoder(num_streams, max_words=None)
    words, n_words = enc(x, y, p, t, counts, reset=None)
      x, y, p: int64 / int32 / int16 [S, chunk_events], t: int64 / int32 (microseconds), the columns `EventQueue.push` takes; counts:
        int64 [S], the events at the head of each row; reset: uint8 / bool [S], non-zero for the rows whose encoder state is zeroed
        before this chunk: a new recording.
      -> words int16 [S, max_words], the 16 bits of each word (what `Evt3Decoder` and `push_evt3` take), n_words int64 [S] the words at
        the head of each row.  The tensors are the encoder's staging: the next call overwrites them.
    words, n_words = enc.encode_dat(records, counts, reset=None)
      records: int32 [S, chunk_events, 2], Prophesee's packed Event2D records as `EventQueue.push_dat` takes them: DAT -> EVT 3.0.
    Nothing is dropped: a time below the row's running maximum is raised to it, x and y are clamped to 0 .. 2047, p becomes p != 0,
    and each such event is counted.  The state after a chunk (have, t_last, y_last) is the state before the next one, per row: the
    words of the chunks of a recording, one after the other, decode to its events wherever it was cut (the words themselves depend on
    the cuts: a cut ends a vector group).  A fresh decoder starts its wrap count at 0, so it returns t - ((t0 >> 24) << 24) with t0 the
    row's first event: inherent to the format's 24-bit clock.
    max_words: the words one row's chunk may give.  The default, 5 * chunk_events + 1024, covers the 5 words an event can need and the
    TIME_HIGH keep-alives (one per 2^22 us) of over an hour of silence per chunk; a longer gap needs an explicit max_words.  A row
    that does not fit is refused whole: n_words 0, its state as it was, and `errors()` reports it.
    `errors()` -> (times raised to the running maximum, events with x, y or p clamped, rows refused for lack of room, 0), accumulated
    until `reset()`; `reset(streams=None)` zeroes the encoder state of the rows (default: all, and the counters).  `state` is int64
    [S, 4]: have, t_last, y_last, 0.
    The state and the staging are allocated by the first un-captured call, never during capture; afterwards nothing is allocated and
    nothing synchronises.  One call is 2 launches whatever S and the sizes are."""

    _STATE_WORDS, _WS_BYTES, _ENCODE, _ENCODE_DAT = "EVT3_ENC_STATE_WORDS", "sast_evt3enc_ws_bytes", "sast_evt3enc_encode", "sast_evt3enc_encode_dat"
    _word_dtype = torch.int16

    def _room(self, chunk_events: int) -> int:
        return 5 * chunk_events + 1024


def evt3_raw_header(height: int, width: int) -> bytes:
    """The ASCII header of a Prophesee .raw file of EVT 3.0 words for a sensor of `height` x `width` pixels.  Host only.  The bytes,
    followed by the little-endian bytes of `words[s, :n_words[s]]` of `Evt3Encoder` chunk after chunk, are a .raw file; `raw_header`
    reads them back as format "evt3", that geometry and the offset of the first word.  The lines are this project's choice of the
    fields such files carry (parity with the Metavision SDK's writer is unpinned)."""
    height, width = int(height), int(width)
    if not (1 <= height <= 2048 and 1 <= width <= 2048):
        raise ValueError("sast_amd.events: an EVT 3.0 sensor has 1 .. 2048 rows and columns")
    return (f"% evt 3.0\n% format EVT3;height={height};width={width}\n% geometry {width}x{height}\n"
            f"% generator sast_amd.events.Evt3Encoder\n% end\n").encode("ascii")


# version -> (the library's code, word dtypes, events one word can give, the words in the dtype message)
_EVT2_VERSIONS = {
    "2.0": (L.EVT2_V20, tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None), 1, "(one EVT 2.0 word each)"),
    "2.1": (L.EVT2_V21, (torch.int64,), 32, "(one EVT 2.1 word each)"),
}


def _evt2_version(version) -> str:
    if version not in _EVT2_VERSIONS:
        raise ValueError(f"sast_amd.events: version must be one of {tuple(_EVT2_VERSIONS)}, got {version!r}")
    return version


class Evt2Decoder(_EventDecoder):
    """Prophesee EVT 2.0 / EVT 2.1 sensor words -> event columns on the device (csrc/k_evt2.hip; the format tables and the decode rule
    are in include/sast_hip.h and INTEGRATION.md §3b; parity with the Metavision SDK's decoder is unpinned, the SDK is not a
    dependency: what is pinned is the sequential model of tests/evt2_model.py).

    dec = Evt2Decoder(num_streams, max_events=None, version="2.0")
    x, y, p, t, n = dec(words, counts, reset=None)
      words: version "2.0": int32 (uint32 where torch has it) [S, chunk_words], one word is at most one event; version "2.1": int64
        [S, chunk_words], one word is a 32-pixel vector, the 64-bit word as a little-endian integer (a stream whose 32-bit halves
        arrive in the other order is the caller's to swap: `words.view(torch.int32).view(S, -1, 2).flip(-1)`).  The raw words of S
        sensors side by side, cut anywhere (`raw_header` finds the end of a .raw file's ASCII header); counts: int64 [S], the words
        at the head of each row; reset: uint8 / bool [S], non-zero for the rows whose decoder state (the time base) is zeroed before
        this chunk: a new recording.
      -> x, y, p int16 [S, max_events], t int64 [S, max_events] (microseconds, wraps of the 34-bit sensor clock unrolled), n int64 [S]
        the events at the head of each row: what `EventQueue.push` / `EventStreams` take.  The tensors are the decoder's staging
        columns: the next call overwrites them.  An EVT 2.1 vector may reach past column 2047 (x up to 2078): x is stored as written.
    The state after a chunk is the state before the next one, per row: a stream decoded in chunks cut at any word gives the events of
    the stream decoded whole.  max_events: the events one row's chunk may give (default chunk_words for "2.0", 32 * chunk_words for
    "2.1", which can never drop one); of a row with more, the first max_events are kept and the rest counted.  `errors()`, `reset()`
    and the counters' meaning and order are `Evt3Decoder`'s.  `state` is int64 [S, 4]: high, wraps, have_high, 0.
    The state and the staging columns are allocated by the first un-captured call, never during capture; afterwards nothing is
    allocated and nothing synchronises.  One call is 2 launches whatever S and the sizes are."""

    _STATE_WORDS, _WS_BYTES, _DECODE = "EVT2_STATE_WORDS", "sast_evt2_ws_bytes", "sast_evt2_decode"

    def __init__(self, num_streams: int, max_events: Optional[int] = None, version: str = "2.0"):
        self.version = _evt2_version(version)
        code, self._dtypes, self.fanout, self._what = _EVT2_VERSIONS[self.version]
        self._EXTRA = (code,)
        super().__init__(num_streams, max_events)


class Evt2Encoder(_EventEncoder):
    """Event columns or packed Event2D records -> Prophesee EVT 2.0 / EVT 2.1 sensor words on the device (csrc/k_evt2_enc.hip; the word
    tables and the canonical rule are in include/sast_hip.h and INTEGRATION.md §3b; parity with the Metavision SDK's encoder is
    unpinned, the SDK is not a dependency: what is pinned is the sequential model of tests/evt2_encoder_model.py, and that
    `Evt2Decoder` gives the events back).

    enc = Evt2Encoder(num_streams, max_words=None, version="2.0")
    words, n_words = enc(x, y, p, t, counts, reset=None)
      x, y, p: int64 / int32 / int16 [S, chunk_events], t: int64 / int32 (microseconds), the columns `EventQueue.push` takes; counts:
        int64 [S], the events at the head of each row; reset: uint8 / bool [S], non-zero for the rows whose encoder state is zeroed
        before this chunk: a new recording.
      -> words [S, max_words], int32 for version "2.0" (one word per event) and int64 for "2.1" (one word per group of up to 32 events
        of one time, row and polarity inside 32 aligned columns): what `Evt2Decoder` and `push_evt2` take; n_words int64 [S] the words
        at the head of each row.  The tensors are the encoder's staging: the next call overwrites them.
    words, n_words = enc.encode_dat(records, counts, reset=None)
      records: int32 [S, chunk_events, 2], Prophesee's packed Event2D records as `EventQueue.push_dat` takes them: DAT -> EVT 2.x.
    Nothing is dropped: a time below the row's running maximum is raised to it, x and y are clamped to 0 .. 2047, p becomes p != 0,
    and each such event is counted.  The state after a chunk (have, t_last) is the state before the next one, per row: the words of
    the chunks of a recording, one after the other, decode to its events wherever it was cut (the words of "2.1" depend on the cuts: a
    cut ends a group).  A fresh decoder starts its wrap count at 0, so it returns t - ((t0 >> 34) << 34) with t0 the row's first
    event: inherent to the format's 34-bit clock.
    max_words: the words one row's chunk may give.  The default, 2 * chunk_events + 16, covers the 2 words an event can need and the
    TIME_HIGH keep-alives (one per 2^32 us) of about 19 hours of silence per chunk; a longer gap needs an explicit max_words.  A row
    that does not fit is refused whole: n_words 0, its state as it was, and `errors()` reports it.
    `errors()`, `reset(streams=None)` and the counters are `Evt3Encoder`'s.  `state` is int64 [S, 4]: have, t_last, 0, 0.
    The state and the staging are allocated by the first un-captured call, never during capture; afterwards nothing is allocated and
    nothing synchronises.  There is no CPU fallback.  One call is 2 launches whatever S and the sizes are."""

    _STATE_WORDS, _WS_BYTES, _ENCODE, _ENCODE_DAT = "EVT2_ENC_STATE_WORDS", "sast_evt2enc_ws_bytes", "sast_evt2enc_encode", "sast_evt2enc_encode_dat"

    def __init__(self, num_streams: int, max_words: Optional[int] = None, version: str = "2.0"):
        self.version = _evt2_version(version)
        self._EXTRA = (_EVT2_VERSIONS[self.version][0],)
        self._word_dtype = torch.int32 if self.version == "2.0" else torch.int64
        super().__init__(num_streams, max_words)

    def _room(self, chunk_events: int) -> int:
        return 2 * chunk_events + 16


def evt2_raw_header(height: int, width: int, version: str = "2.0") -> bytes:
    """The ASCII header of a Prophesee .raw file of EVT 2.0 / EVT 2.1 words for a sensor of `height` x `width` pixels.  Host only.  The
    bytes, followed by the little-endian bytes of `words[s, :n_words[s]]` of `Evt2Encoder` chunk after chunk, are a .raw file;
    `raw_header` reads them back as format "evt2" / "evt21", that geometry and the offset of the first word.  The lines are this
    project's choice of the fields such files carry (parity with the Metavision SDK's writer is unpinned)."""
    version = _evt2_version(version)
    height, width = int(height), int(width)
    if not (1 <= height <= 2048 and 1 <= width <= 2048):
        raise ValueError("sast_amd.events: an EVT 2 sensor has 1 .. 2048 rows and columns")
    name = "EVT2" if version == "2.0" else "EVT21"
    return (f"% evt {version}\n% format {name};height={height};width={width}\n% geometry {width}x{height}\n"
            f"% generator sast_amd.events.Evt2Encoder\n% end\n").encode("ascii")


FILTER_MODES = {"activity": L.EVFILTER_ACTIVITY, "contrast": L.EVFILTER_CONTRAST}


class EventFilter:
    """Event-level noise filters on the device, between decode and accumulate (csrc/k_evfilter.hip; the rule is in include/sast_hip.h
    and INTEGRATION.md §3b; it is this project's: parity with the Metavision SDK's ActivityNoiseFilterAlgorithm and
    SpatioTemporalContrastAlgorithm is unpinned, the SDK is not a dependency: what is pinned is the sequential model of
    tests/event_filter_model.py).

    f = EventFilter(num_streams, height, width, mode="activity" | "contrast", threshold_us=10_000, radius=1)
    x, y, p, t, n = f(x, y, p, t, counts, reset=None)
      x, y, p: int64 / int32 / int16 [S, chunk_cap], t: int64 / int32 (microseconds), the columns `EventQueue.push` takes (a decoder's
        staging columns among them); counts: int64 [S], the events at the head of each row; reset: uint8 / bool [S], non-zero for the
        rows that start a new recording with this chunk: surface -1, carry and the row's seen / kept 0 first.
      -> x, y, p int16 [S, chunk_cap], t int64 [S, chunk_cap], n int64 [S] the kept events at the head of each row, in arrival order:
        what `EventQueue.push` takes.  The tensors are the filter's staging columns: the next call overwrites them.
    x, y, p, t, n = f.filter_dat(records, counts, reset=None)
      records: int32 [S, chunk_cap, 2], Prophesee's packed Event2D records as `EventQueue.push_dat` takes them.
    Per row, in arrival order: t' is the running maximum of the times from the filter's own carry `t_last` (the queue's correction, so
    the queue's is the identity on what comes out); `surface` holds per pixel -1 or 2 * t' + (p > 0) of the last event there, kept or
    not.  mode="activity": an event is kept iff another pixel within Chebyshev distance `radius` (1 .. 3) saw an event at most
    threshold_us before (<=), polarity ignored.  mode="contrast": iff its own pixel's last event had the same polarity and was at most
    threshold_us before.  Events outside the sensor are dropped and counted (`errors()`), they still advance t'.  The decision never
    depends on an earlier decision, so a recording cut into chunks anywhere gives the events and state of the recording in one call.
    State, device tensors allocated by the first ordinary call and never during capture: surface int64 [S, H, W], t_last int64 [S],
    seen / kept int64 [S] (cumulative per row), err int32 [1].  `reset(streams=None)` is the host-side form of `reset`: those rows
    (default: all, and the counter) start over.  One call is FILTER_LAUNCHES launches of the library and one device radix sort over
    S * chunk_cap keys whose passes depend on the shapes alone; after one un-captured warm-up call with the same shapes nothing is
    allocated and nothing synchronises, so a call can be captured in a graph.  There is no CPU fallback."""

    FILTER_LAUNCHES = L.EVFILTER_LAUNCHES

    def __init__(self, num_streams: int, height: int, width: int, mode: str = "activity", threshold_us: int = 10_000, radius: int = 1):
        self.num_streams = F.stream_count(num_streams, "events")
        if not (1 <= int(height) <= 32767 and 1 <= int(width) <= 32767):
            raise ValueError("sast_amd.events: EventFilter gives x and y as int16: height and width must be in 1 .. 32767")
        if mode not in FILTER_MODES:
            raise ValueError(f"sast_amd.events: mode must be one of {tuple(FILTER_MODES)}, got {mode!r}")
        if isinstance(threshold_us, bool) or not isinstance(threshold_us, int) or not 0 <= threshold_us < 2 ** 62:
            raise ValueError("sast_amd.events: threshold_us must be an int in 0 .. 2^62 - 1")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 3:
            raise ValueError("sast_amd.events: radius must be an int in 1 .. 3")
        self.height, self.width, self.mode, self.threshold_us, self.radius = int(height), int(width), mode, threshold_us, radius
        self.surface = self.t_last = self.seen = self.kept = self.err = self.counts = self.x = self.y = self.p = self.t = None
        self._ws = self._args = None

    def _buffers(self, dev, chunk_cap: int):
        S = self.num_streams
        if self.surface is None:
            F.not_capturing("events")
            self.surface = torch.full((S, self.height, self.width), -1, dtype=torch.int64, device=dev)
            self.t_last, self.seen, self.kept, self.counts = (torch.zeros(S, dtype=torch.int64, device=dev) for _ in range(4))
            self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        F.lives_on("the filter's state", self.surface.device, "the call's tensors", dev, "events")
        if self.x is None or self.x.shape[1] < chunk_cap:
            F.not_capturing("events")
            need = int(L.lib().sast_evfilter_ws_bytes(S, chunk_cap, self.height, self.width))
            if need == 0:
                raise ValueError(f"sast_amd.events: unsupported filter shapes (num_streams={S}, chunk capacity {chunk_cap}, "
                                 f"{self.height}x{self.width}): the sort keys do not fit 63 bits")
            room = max(chunk_cap, 1)
            self.x, self.y, self.p = (torch.zeros(S, room, dtype=torch.int16, device=dev) for _ in range(3))
            self.t = torch.zeros(S, room, dtype=torch.int64, device=dev)
            self._ws = torch.zeros(need, dtype=torch.uint8, device=dev)
            a = self._args = L.SastEvFilterArgs()
            a.surface, a.t_last, a.seen, a.kept = self.surface.data_ptr(), self.t_last.data_ptr(), self.seen.data_ptr(), self.kept.data_ptr()
            a.err, a.ws, a.ws_bytes = self.err.data_ptr(), self._ws.data_ptr(), need
            a.x, a.y, a.p, a.t, a.out_counts = self.x.data_ptr(), self.y.data_ptr(), self.p.data_ptr(), self.t.data_ptr(), self.counts.data_ptr()
            a.out_capacity, a.threshold_us = room, self.threshold_us
            a.S, a.height, a.width, a.mode, a.radius = S, self.height, self.width, FILTER_MODES[self.mode], self.radius
        return self._args

    def errors(self) -> Tuple[int]:
        """(events outside the sensor,) since the last reset() (synchronises)"""
        return F.counters(self.err, 1)

    def reset(self, streams=None):
        """new recordings, from the host: the surface of `streams` (default: all of them) back to -1, their carry and their seen / kept
        counts to 0; with streams=None the error counter is cleared as well"""
        F.reset_rows((self.t_last, self.seen, self.kept), self.err, streams, self.num_streams, "events")
        if self.surface is not None:
            if streams is None:
                self.surface.fill_(-1)
            elif len(list(streams)):
                self.surface[torch.tensor([int(s) for s in streams], dtype=torch.int64, device=self.surface.device)] = -1

    def _filter(self, entry, head, chunk_cap, counts, reset, tensors):
        S = self.num_streams
        F.counts_reset(counts, reset, S, "events")
        if S * chunk_cap > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * chunk capacity must be below 2^31")
        _need_gpu(*tensors, counts, reset)
        F.same_device("events", "the chunk, counts and reset", *tensors, counts, reset)
        a = self._buffers(counts.device, chunk_cap)
        # an empty chunk has no storage: any valid device pointer will do, the kernels read no event
        head = [h or counts.data_ptr() for h in head[:len(tensors)]] + list(head[len(tensors):])
        L.check(getattr(L.lib(), entry)(C.byref(a), *head, counts.data_ptr(), chunk_cap, None if reset is None else reset.data_ptr(),
                                        _stream()), entry[len("sast_"):])
        return self.x, self.y, self.p, self.t, self.counts

    def __call__(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor,
                 reset: Optional[torch.Tensor] = None):
        codes = F.event_columns(x, y, p, t, self.num_streams, "events", cap_name="chunk capacity")
        return self._filter("sast_evfilter_apply", [c.data_ptr() for c in (x, y, p, t)] + list(codes), x.shape[1], counts, reset, [x, y, p, t])

    def filter_dat(self, records: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None):
        F.tensor_arg(records, "records", "events", (torch.int32,), (("num_streams", self.num_streams), "chunk capacity", 2),
                     "(two words per Event2D record)", empty_ok=True, dtype_error=TypeError)
        return self._filter("sast_evfilter_apply_dat", [records.data_ptr()], records.shape[1], counts, reset, [records])


class RawHeader(NamedTuple):
    """what `raw_header` reads: format "evt2" / "evt21" / "evt3" / None, width and height (None where the header names none), offset the
    index of the first data byte, fields {key: the rest of the line} of every header line"""
    format: Optional[str]
    width: Optional[int]
    height: Optional[int]
    offset: int
    fields: Dict[str, str]


_RAW_FORMATS = {"EVT2": "evt2", "EVT20": "evt2", "EVT21": "evt21", "EVT3": "evt3", "EVT30": "evt3",
                "2": "evt2", "20": "evt2", "21": "evt21", "3": "evt3", "30": "evt3"}


def _to_int(text: str) -> Optional[int]:
    text = text.strip()
    return int(text) if text.isdigit() else None


def raw_header(data) -> RawHeader:
    """The ASCII header of a Prophesee .raw file -> RawHeader(format, width, height, offset, fields).  Host only: `data` is bytes, a
    bytearray or a memoryview holding the head of the file; the sensor words start at data[offset:].

    The header is the run of lines starting with '%' at the head of the file.  The line "% end" ends it right after its newline,
    whatever byte follows (a data byte may be 0x25, '%'); without a "% end" line it ends at the first line that does not start with
    '%'.  A '\\r' before the newline is dropped.  `fields` maps each line's key (its first word behind the '%') to the rest of the
    line; the "% end" line is no field.  format: from "% format EVT3;height=720;width=1280" (the value up to the first ';', then
    key=value pairs), failing that from "% evt 3.0"; width and height: from the pairs of the format field, failing that from
    "% geometry 1280x720", else None.  A buffer that ends inside the header (in the middle of a line, or behind a header line that
    is not "% end" with nothing after it to tell whether another follows) raises ValueError: more bytes are needed.
    This is this project's reading of such files; parity with the Metavision SDK's reader is unpinned (the SDK is not a dependency)."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError(f"sast_amd.events: raw_header takes bytes, a bytearray or a memoryview, got a {type(data).__name__}")
    buf = bytes(data)
    more = "sast_amd.events: the buffer ends inside the .raw header: more bytes are needed"
    fields: Dict[str, str] = {}
    at = 0
    while True:
        if at >= len(buf):
            raise ValueError(more)
        if buf[at] != 0x25:
            break
        nl = buf.find(b"\n", at)
        if nl < 0:
            raise ValueError(more)
        line = buf[at + 1:nl]
        at = nl + 1
        if line.endswith(b"\r"):
            line = line[:-1]
        key, _sep, rest = line.decode("latin-1").strip().partition(" ")
        if key == "end" and not rest.strip():
            break
        if key:
            fields[key] = rest.strip()
    fmt = width = height = None
    if "format" in fields:
        name, *pairs = fields["format"].split(";")
        fmt = _RAW_FORMATS.get(name.strip().upper().replace(".", ""))
        geo = dict(pair.split("=", 1) for pair in pairs if "=" in pair)
        width, height = _to_int(geo.get("width", "")), _to_int(geo.get("height", ""))
    if fmt is None and "evt" in fields:
        fmt = _RAW_FORMATS.get(fields["evt"].strip().replace(".", ""))
    if (width is None or height is None) and "geometry" in fields:
        w, _x, h = fields["geometry"].lower().partition("x")
        if _to_int(w) is not None and _to_int(h) is not None:
            width, height = _to_int(w), _to_int(h)
    return RawHeader(fmt, width, height, at, fields)


_QUEUE_ERRORS = ("{} invalid events (x or y outside the sensor, or a polarity outside 0..1); they were skipped",
                 "{} windows hold more events than window_capacity; they were left empty",
                 "{} events were dropped: their row of the queue was full (capacity >= 2 x the row's live events right after a `frames` call + all events pushed between two `frames` calls never drops)",
                 "{} late windows: they end before one the row already gave, and events they need were retired")


class EventQueue(_Windowed):
    """Device-resident event retention across chunks: push chunks of any size as they arrive, ask for windows as their ends pass.

    q = EventQueue(num_streams, capacity, height, width, ..., duration_us=D | num_events=N, filter=None)
    q.push(x, y, p, t, counts, reset=None)      chunk columns [S, chunk_cap] (x, y, p: int64 / int32 / int16; t: int64 / int32),
                                                counts int64 [S]: row s appends the first counts[s] events of chunk row s
    q.push_dat(records, counts, reset=None)     int32 [S, chunk_cap, 2]: Prophesee's packed Event2D records as the reference's reader
                                                takes them (EV_TYPE, utils/evaluation/prophesee/io/dat_events_tools.py:18-50):
                                                word 0 is t, an UNSIGNED 32-bit count of microseconds; word 1 gives x = w & 16383,
                                                y = (w >> 14) & 16383, p = (w >> 28) & 1, bits 29-31 ignored.  Decoded in the append
                                                kernel: no unpacked copy exists.  The 32-bit clock wraps after ~71.6 minutes; it is
                                                NOT unwrapped (the reference does not either): after a wrap the time correction holds
                                                every timestamp at the maximum before it.
    q.push_evt3(words, counts, reset=None)      int16 / uint16 [S, chunk_words]: raw EVT 3.0 sensor words, counts in words, cut at any
                                                word (`Evt3Decoder`: the stateful decode runs on the device, 2 launches, in front of
                                                the append); `evt3_errors()` gives the decoder's three counters.
    q.push_evt2(words, counts, reset=None, max_events=None, version="2.0")
                                                int32 [S, chunk_words] raw EVT 2.0 words, or with version="2.1" int64 [S, chunk_words]
                                                raw EVT 2.1 words (`Evt2Decoder`, 2 launches in front of the append);
                                                `evt2_errors()` gives that decoder's three counters.
    filter: an `EventFilter` for the same streams and sensor: every push then sends its events (the decoder's staging columns and
                                                device-side counts for raw words) through it in front of the append -- FILTER_LAUNCHES more
                                                launches and one radix sort per push; `reset` and `reset(streams=)` reach it.  The
                                                filter sees sensor coordinates (`downsample_by_2` happens in the frames).  None: the
                                                queue runs the launches and gives the bytes it gives without one.
    frames = q.frames(ends_us, out=None, check=False)    ends_us int64 [S] or [T, S] -> frames as `EventStreams` returns them
    q.reset(streams=None); q.errors(); q.get_shape()

    The frames equal, byte for byte, what `EventStreams` gives for the whole recording in one buffer.  Geometry, representations, `out`,
    `window_capacity` (default: capacity), frame dtype and shape are `EventStreams`'.

    State, all device tensors, allocated by the first ordinary call and never during capture: x, y, p int16 [S, capacity] (narrowed
    with saturation: x = 65541 stays outside the sensor and is counted invalid, it is not drawn in column 5), t int64 [S, capacity]
    (corrected: the running maximum from `t_last[s]`, carried on), head, count int64 [S] (row s's live events are [head[s], count[s])),
    t_last int64 [S], retired / retired_t int64 [S] (how many events the row retired, the corrected time of the last one), err int32 [4]
    (invalid events, windows over window_capacity, events dropped for lack of room, late windows).

    push: `reset[s] != 0` (uint8 / bool [S], device) first empties row s and zeroes its carry and retirement record (`reset(streams=...)`
    is the host-side form).  Of a chunk that does not fit, the first events that do are stored, the rest are counted in err[2]; the carry
    advances over the stored ones only.
    frames: windows are searched in each row's live events by `EventStreams`' rules (duration: end - D <= t <= end; count: the last N
    events with t <= end, stopping at the row's first live event); `last_bounds` (int64 [T*S, 2]) holds flat indices into the
    [S * capacity] storage as it was during the call, so num_streams * capacity < 2^31.  Then the row retires: it keeps its events from
    the start of its LAST window (step T-1), everything before is gone.  A row is moved to the front of its storage only when its live
    events fit into the freed slots in front of them (live <= head: source and destination are disjoint, the copy needs no scratch);
    otherwise it keeps filling.  Sizing rule: capacity >= 2 x R + P never drops an event, with R the most live events a row has right
    after a `frames` call (its last window plus whatever was already pushed beyond that window's end) and P the most events the row is
    pushed between two `frames` calls (one chunk only if `frames` follows every push): a row that just missed the move has head = R - 1
    slots unused in front of R live events, and fills up to 2 R - 1 + P before the next retirement.

    Contract: (1) ends_us[., s] is non-decreasing over steps and over calls; (2) a window is asked for once every event with t <= end
    has been pushed -- an event later than `end` has arrived, or the recording is over.  A window that breaks (1) after events were
    retired is counted in err[3] (duration: the row's last retired time is >= end - D; count: the window reaches the row's first live
    event with fewer than N events, and the row has retired events); its frame is whatever the live events give.

    check=True: after the call the counters are read (this synchronises) and cleared, and ValueError names the first non-zero one.
    Unlike `EventFrames` / `EventStreams`, which clear the counters BEFORE a checked call and so report that call alone, this reports
    everything since the counters were last cleared: drops happen in `push`, which has no check of its own, and must not be lost.
    After one un-captured warm-up call of each method with the same shapes nothing synchronises and nothing but `out` is allocated, so
    push + frames (+ augmentor + backbone) can be captured in one graph and replayed on new chunks, counts, ends and reset flags written
    into the same tensors.  Launches, whatever S, T and the chunk size are: 2 per push (partial maxima; scan + decode + append), 7 per
    frames (1 window search, 4 frame launches, 2 retire: plan, compaction)."""

    PUSH_LAUNCHES = 2
    PUSH_EVT3_LAUNCHES = Evt3Decoder.DECODE_LAUNCHES + PUSH_LAUNCHES
    PUSH_EVT2_LAUNCHES = Evt2Decoder.DECODE_LAUNCHES + PUSH_LAUNCHES
    FRAMES_LAUNCHES = 7

    def __init__(self, num_streams: int, capacity: int, height: int, width: int, bins: int = 10, count_cutoff: Optional[int] = 10,
                 fastmode: bool = True, duration_us: Optional[int] = None, num_events: Optional[int] = None, downsample_by_2: bool = False,
                 window_capacity: Optional[int] = None, representation: str = "stacked_histogram", filter: Optional[EventFilter] = None):
        super().__init__(bins, height, width, count_cutoff, fastmode, downsample_by_2, representation, duration_us, num_events, True,
                         window_capacity)
        if int(height) > 32767 or int(width) > 32767:
            raise ValueError("sast_amd.events: EventQueue keeps x and y as int16: height and width must be <= 32767")
        F.stream_count(num_streams, "events")
        if int(capacity) < 1:
            raise ValueError("sast_amd.events: capacity must be >= 1")
        if int(num_streams) * int(capacity) > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * capacity must be below 2^31")
        self.num_streams, self.capacity = int(num_streams), int(capacity)
        self.x = self.y = self.p = self.t = self.head = self.count = self.retired = self.retired_t = None
        self._args = None
        self.evt3: Optional[Evt3Decoder] = None       # made by the first push_evt3
        self.evt2: Optional[Evt2Decoder] = None       # made by the first push_evt2
        if filter is not None:
            if not isinstance(filter, EventFilter):
                raise TypeError(f"sast_amd.events: filter must be a sast_amd.events.EventFilter (or None), got a {type(filter).__name__}")
            if (filter.num_streams, filter.height, filter.width) != (self.num_streams, self.height, self.width):
                raise ValueError(f"sast_amd.events: the filter is for {filter.num_streams} streams of {filter.height}x{filter.width}, the queue "
                                 f"for {self.num_streams} of {self.height}x{self.width}")
        self.filter = filter

    def _storage(self, dev):
        """the queue's state on `dev` (allocated by the first ordinary call)"""
        if self._args is not None:
            F.lives_on("the queue's state", self.t.device, "the call's tensors", dev, "events")
        else:
            F.not_capturing("events")
            S, cap = self.num_streams, self.capacity
            self.x, self.y, self.p = (torch.zeros(S, cap, dtype=torch.int16, device=dev) for _ in range(3))
            self.t = torch.zeros(S, cap, dtype=torch.int64, device=dev)
            self.head, self.count, self.t_last, self.retired, self.retired_t = (torch.zeros(S, dtype=torch.int64, device=dev) for _ in range(5))
            self.err = torch.zeros(4, dtype=torch.int32, device=dev)
            self._state = {"ws": torch.zeros(int(L.lib().sast_evqueue_ws_count(S)), dtype=torch.int64, device=dev)}
            a = self._args = L.SastEvQueueArgs()
            a.x, a.y, a.p, a.t = self.x.data_ptr(), self.y.data_ptr(), self.p.data_ptr(), self.t.data_ptr()
            a.head, a.count, a.t_last = self.head.data_ptr(), self.count.data_ptr(), self.t_last.data_ptr()
            a.retired, a.retired_t, a.err, a.ws = self.retired.data_ptr(), self.retired_t.data_ptr(), self.err.data_ptr(), self._state["ws"].data_ptr()
            a.capacity, a.S = cap, S
        return self._args

    def errors(self) -> Tuple[int, int, int, int]:
        """(invalid events, windows over capacity, dropped events, late windows) since they were last cleared (synchronises)"""
        return F.counters(self.err, 4)

    def reset(self, streams=None):
        """new recordings, from the host: rows `streams` (default: all of them) are emptied, their carry and retirement record zeroed;
        with streams=None the error counters are cleared as well"""
        for dec in (self.evt3, self.evt2, self.filter):
            if dec is not None:
                dec.reset(streams)
        F.reset_rows((self.head, self.count, self.t_last, self.retired, self.retired_t), self.err, streams, self.num_streams, "events")

    def _push(self, ptrs, codes, chunk_cap, counts, reset, tensors):
        F.counts_reset(counts, reset, self.num_streams, "events")
        _need_gpu(*tensors, counts, reset)
        F.same_device("events", "the chunk, counts and reset", *tensors, counts, reset)
        if self.num_streams * chunk_cap > 2 ** 31 - 1:
            raise ValueError("sast_amd.events: num_streams * chunk capacity must be below 2^31")
        a = self._storage(counts.device)
        # an empty chunk has no storage: any valid device pointer will do, the kernels read no event
        ptrs = [v or self.t.data_ptr() for v in ptrs]
        L.check(L.lib().sast_evqueue_push(C.byref(a), *ptrs, *codes, counts.data_ptr(), chunk_cap, None if reset is None else reset.data_ptr(),
                                          _stream()), "evqueue_push")

    def push(self, x: torch.Tensor, y: torch.Tensor, p: torch.Tensor, t: torch.Tensor, counts: torch.Tensor,
             reset: Optional[torch.Tensor] = None) -> None:
        if self.filter is not None:
            x, y, p, t, counts = self.filter(x, y, p, t, counts, reset)
        codes = F.event_columns(x, y, p, t, self.num_streams, "events", cap_name="chunk capacity")
        self._push([c.data_ptr() for c in (x, y, p, t)], codes, x.shape[1], counts, reset, [x, y, p, t])

    def push_dat(self, records: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None) -> None:
        F.tensor_arg(records, "records", "events", (torch.int32,), (("num_streams", self.num_streams), "chunk capacity", 2),
                     "(two words per Event2D record)", empty_ok=True, dtype_error=TypeError)
        if self.filter is not None:
            x, y, p, t, n = self.filter.filter_dat(records, counts, reset)
            return self._push([c.data_ptr() for c in (x, y, p, t)], [L.DT_I16, L.DT_I16, L.DT_I16, L.DT_I64], x.shape[1], n, reset, [x, y, p, t])
        self._push([records.data_ptr()] * 4, [L.EVQUEUE_DT_DAT] * 4, records.shape[1], counts, reset, [records])

    def _push_words(self, name, cls, fixed, max_events, words, counts, reset):
        """raw words through the queue's decoder `name`, made by the first call with the parameters `fixed` and max_events, which a
        later call may not change; then the append of `push` on its staging columns and device-side event counts"""
        dec = getattr(self, name)
        if dec is None:
            dec = cls(self.num_streams, max_events, **fixed)
            setattr(self, name, dec)
        for key, value in fixed.items():
            if value != getattr(dec, key):
                raise ValueError(f"sast_amd.events: the queue's decoder was made with {key}={getattr(dec, key)!r}, got {value!r}")
        if max_events is not None and int(max_events) != dec.max_events:
            raise ValueError(f"sast_amd.events: the queue's decoder was made with max_events={dec.max_events}, got {max_events}")
        F.counts_reset(counts, reset, self.num_streams, "events")
        x, y, p, t, n = dec(words, counts, reset)
        self.push(x, y, p, t, n, reset)

    def push_evt3(self, words: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None,
                  max_events: Optional[int] = None) -> None:
        """raw EVT 3.0 sensor words (int16 / uint16 [S, chunk_words], counts int64 [S] in WORDS) as `Evt3Decoder` takes them: the
        decode (2 launches) into the decoder's staging columns, then the append of `push` on those columns and the decoder's device-side
        event counts (2 launches).  reset[s] != 0 zeroes row s's decoder state and empties its queue row together.  max_events: the
        decoder's staging per row, fixed by the first call (default 12 * chunk_words: never drops)."""
        self._push_words("evt3", Evt3Decoder, {}, max_events, words, counts, reset)

    def evt3_errors(self) -> Tuple[int, int, int]:
        """the decoder's counters of `push_evt3`: (events before the first TIME_HIGH, unknown words, events dropped for lack of
        staging) (synchronises); `errors()` keeps the queue's four"""
        return (0, 0, 0) if self.evt3 is None else self.evt3.errors()

    def push_evt2(self, words: torch.Tensor, counts: torch.Tensor, reset: Optional[torch.Tensor] = None,
                  max_events: Optional[int] = None, version: str = "2.0") -> None:
        """raw EVT 2.0 (int32 [S, chunk_words]) or, with version="2.1", EVT 2.1 (int64 [S, chunk_words]) sensor words, counts int64 [S]
        in WORDS, as `Evt2Decoder` takes them: the decode (2 launches) into the decoder's staging columns, then the append of `push` on
        those columns and the decoder's device-side event counts (2 launches).  reset[s] != 0 zeroes row s's decoder state and empties
        its queue row together.  version and max_events (the decoder's staging per row; default chunk_words / 32 * chunk_words: never
        drops) are fixed by the first call: a later call with another of either raises ValueError."""
        self._push_words("evt2", Evt2Decoder, {"version": _evt2_version(version)}, max_events, words, counts, reset)

    def evt2_errors(self) -> Tuple[int, int, int]:
        """the decoder's counters of `push_evt2`: (events before the first TIME_HIGH, unknown words, events dropped for lack of
        staging) (synchronises); `errors()` keeps the queue's four"""
        return (0, 0, 0) if self.evt2 is None else self.evt2.errors()

    def frames(self, ends_us: torch.Tensor, out: Optional[torch.Tensor] = None, check: bool = False) -> torch.Tensor:
        S, cap = self.num_streams, self.capacity
        T, wcap, shape = self._frames_shape(ends_us, S, cap)
        _need_gpu(ends_us, out)
        dev = ends_us.device
        out = F.frames_out(out, shape, self.frame_dtype, dev, "events", "out", "the queue's")
        a = self._storage(dev)
        bounds = self._bounds(T * S, dev)
        lib = L.lib()
        L.check(lib.sast_evqueue_window_bounds(C.byref(a), ends_us.data_ptr(), T, self.mode, self.value, bounds.data_ptr(), _stream()),
                "evqueue_window_bounds")
        self.launch([self.x, self.y, self.p, self.t], [L.DT_I16, L.DT_I16, L.DT_I16, L.DT_I64], S * cap, bounds, out, self.err, wcap,
                    clip_negative_polarity=True)
        L.check(lib.sast_evqueue_retire(C.byref(a), bounds.data_ptr(), T, _stream()), "evqueue_retire")
        self.last_bounds = bounds
        if check:
            err = self.errors()
            self.err.zero_()
            for n, msg in zip(err, _QUEUE_ERRORS):
                if n:
                    raise ValueError("sast_amd.events: " + msg.format(n))
        return out
