"""The argument rules of the data front end (sast_amd/_frontend.py), driven directly: for every rule one call that passes and one per way
of failing, with the exception type and the three things a message must hold -- the module in front, the argument's name, the shape
as the caller wrote it.  Then one case per front-end class: a CPU tensor of the wrong shape meets the shape rule, one of the right
shape the library's "no CPU fallback" error.  No GPU is needed: the rules look at shape, dtype and layout only."""
import re

import pytest
import torch

from sast_amd import _frontend as F

I64, I32, I16, U8 = torch.int64, torch.int32, torch.int16, torch.uint8
META = torch.device("meta")


def _raises(kind, *words):
    """pytest.raises whose message must hold every one of `words`"""
    return pytest.raises(kind, match="".join(f"(?=.*{w})" for w in (re.escape(w) for w in words)))


# ------------------------------------------------------------------------------------------------------------------------ tensor_arg
def test_tensor_arg_passes():
    F.tensor_arg(torch.zeros(4, 3, dtype=I32), "rows", "events", (I32,), ("T", 3))
    F.tensor_arg(torch.zeros(4, 3, dtype=I32), "rows", "events", None, (("num_streams", 4), 3))            # any dtype
    F.tensor_arg(torch.zeros(3, dtype=I64), "ends", "labels", (I64,), [(3,), ("T", 3)])                    # one of two ranks
    F.tensor_arg(torch.zeros(2, 3, dtype=I64), "ends", "labels", (I64,), [(3,), ("T", 3)])
    F.tensor_arg(torch.zeros(3, 0, dtype=I16), "words", "events", (I16,), (3, "chunk words"), empty_ok=True)
    F.tensor_arg(torch.zeros(3, dtype=U8, device=META), "out", "events", (U8,), (3,), "on the queue's device", device=META)


@pytest.mark.parametrize("bad, kind, got", [
    (torch.zeros(4, 3, dtype=I64), ValueError, "int64 [4, 3]"),                       # wrong dtype
    (torch.zeros(4, dtype=I32), ValueError, "int32 [4]"),                             # wrong rank
    (torch.zeros(4, 2, dtype=I32), ValueError, "int32 [4, 2]"),                       # wrong length
    (torch.zeros(0, 3, dtype=I32), ValueError, "int32 [0, 3]"),                       # a free size of 0
    (torch.zeros(3, 4, dtype=I32).t(), ValueError, "strides [1, 4]"),                 # not contiguous
    ([[0, 0, 0]], ValueError, "a list"),                                              # not a tensor
    (None, ValueError, "a NoneType"),
], ids=["dtype", "rank", "length", "empty", "strides", "list", "none"])
def test_tensor_arg_fails(bad, kind, got):
    with _raises(kind, "sast_amd.events: rows must be a contiguous int32 tensor of shape [T, 3], T >= 1 (three words a row), got " + got):
        F.tensor_arg(bad, "rows", "events", (I32,), ("T", 3), "(three words a row)")


def test_tensor_arg_variants():
    with _raises(TypeError, "sast_amd.events: words must be a contiguous int16 or int32 tensor of shape [num_streams=3, chunk words], got"):
        F.tensor_arg(torch.zeros(3, 8, dtype=I64), "words", "events", (I16, I32), (("num_streams", 3), "chunk words"), empty_ok=True,
                     dtype_error=TypeError)
    with _raises(ValueError, "words must be", "[num_streams=3, chunk words]", "int16 [2, 8]"):             # the shape stays a ValueError
        F.tensor_arg(torch.zeros(2, 8, dtype=I16), "words", "events", (I16,), (("num_streams", 3), "chunk words"), empty_ok=True,
                     dtype_error=TypeError)
    with _raises(ValueError, "sast_amd.labels: ends must be a contiguous int64 tensor of shape [3] or [T, 3], T >= 1, got int64 [2, 4]"):
        F.tensor_arg(torch.zeros(2, 4, dtype=I64), "ends", "labels", (I64,), [(3,), ("T", 3)])
    with _raises(ValueError, "sast_amd.events: out must be a contiguous uint8 tensor of shape [3] on the queue's device, got a tensor on cpu"):
        F.tensor_arg(torch.zeros(3, dtype=U8), "out", "events", (U8,), (3,), "on the queue's device", device=META)
    with _raises(ValueError, "sast_amd.events: x must be a contiguous tensor of shape [rows=3, capacity], got int64 [3]"):
        F.tensor_arg(torch.zeros(3, dtype=I64), "x", "events", None, (("rows", 3), "capacity"), empty_ok=True)


# --------------------------------------------------------------------------------------------------------------------- event columns
def test_event_columns():
    ev = torch.zeros(3, 16, dtype=I64)
    from sast_amd import _lib as L
    assert F.event_columns(ev, ev.to(I32), ev.to(I16), ev.to(I32), 3, "events") == [L.DT_I64, L.DT_I32, L.DT_I16, L.DT_I32]
    assert len(F.event_columns(ev[:, :0], ev[:, :0], ev[:, :0], ev[:, :0], 3, "events")) == 4              # an empty chunk
    cases = [
        ((ev[:2], ev, ev, ev), ValueError, "x must be", "int64 [2, 16]"),                                  # wrong row count
        ((ev, ev[0], ev, ev), ValueError, "y must be", "int64 [16]"),                                      # wrong rank
        ((ev, ev, ev.t().contiguous().t(), ev), ValueError, "p must be a contiguous", "strides [1, 3]"),   # not contiguous
        ((ev, ev, ev, ev.tolist()), ValueError, "t must be", "a list"),                                    # not a tensor
    ]
    for cols, kind, *words in cases:
        with _raises(kind, "sast_amd.sampling: ", "[rows=3, chunk capacity]", *words):
            F.event_columns(*cols, 3, "sampling", rows_name="rows", cap_name="chunk capacity")
    with _raises(ValueError, "sast_amd.events: x, y, p and t must have the same shape"):                   # wrong length
        F.event_columns(ev, ev, ev, ev[:, :8].contiguous(), 3, "events")
    with _raises(TypeError, "sast_amd.events: x must be one of", "torch.float32"):                         # wrong dtype
        F.event_columns(ev.float(), ev, ev, ev, 3, "events")
    with _raises(TypeError, "sast_amd.events: t must be one of", "torch.int16"):                           # timestamps are not int16
        F.event_columns(ev, ev, ev, ev.to(I16), 3, "events")
    assert F.dtype_code(ev.to(I16), "pol", "events") == L.DT_I16
    with _raises(TypeError, "sast_amd.events: time must be one of"):
        F.dtype_code(ev.to(I16), "time", "events", (I64, I32))


# ---------------------------------------------------------------------------------------------------------------- counts, flags, ends
def test_counts_reset_and_flags():
    counts = torch.zeros(3, dtype=I64)
    F.counts_reset(counts, None, 3, "events")
    F.counts_reset(counts, torch.zeros(3, dtype=U8), 3, "events")
    F.counts_reset(counts, torch.zeros(3, dtype=torch.bool), 3, "events")
    F.flags(None, "final", 3, "online")
    for bad, got in ((counts.to(I32), "int32 [3]"), (counts[:2], "int64 [2]"), (counts.view(3, 1), "int64 [3, 1]"),
                     (torch.zeros(6, dtype=I64)[::2], "strides [2]"), ([0, 0, 0], "a list")):
        with _raises(ValueError, "sast_amd.labels: counts must be a contiguous int64 tensor of shape [3], got " + got):
            F.counts_reset(bad, None, 3, "labels")
    for bad, got in ((counts, "int64 [3]"), (torch.zeros(2, dtype=U8), "uint8 [2]"), (torch.zeros(1, 3, dtype=U8), "uint8 [1, 3]"),
                     (torch.zeros(6, dtype=U8)[::2], "strides [2]"), ((0, 0, 0), "a tuple")):
        with _raises(ValueError, "sast_amd.events: reset must be a contiguous uint8 or bool tensor of shape [3], got " + got):
            F.counts_reset(counts, bad, 3, "events")
        with _raises(ValueError, "sast_amd.online: final must be a contiguous uint8 or bool tensor of shape [3], got " + got):
            F.flags(bad, "final", 3, "online")


def test_stream_count():
    assert F.stream_count(1, "events") == 1 and F.stream_count(65535, "labels") == 65535
    for bad in (0, -2, 65536):
        with _raises(ValueError, "sast_amd.labels: num_streams must be in 1 .. 65535"):
            F.stream_count(bad, "labels")


def test_window_ends():
    assert F.window_ends(torch.zeros(3, dtype=I64), 3, "events") == 1
    assert F.window_ends(torch.zeros(5, 3, dtype=I64), 3, "events") == 5
    for bad, got in ((torch.zeros(3, dtype=I32), "int32 [3]"), (torch.zeros(1, 2, 3, dtype=I64), "int64 [1, 2, 3]"),
                     (torch.zeros(2, 4, dtype=I64), "int64 [2, 4]"), (torch.zeros(0, 3, dtype=I64), "int64 [0, 3]"),
                     (torch.zeros(3, 2, dtype=I64).t(), "strides [1, 2]"), (5, "a int")):
        with _raises(ValueError, "sast_amd.events: ends_us must be a contiguous int64 tensor of shape [3] or [T, 3], T >= 1, got " + got):
            F.window_ends(bad, 3, "events")
    with _raises(ValueError, "sast_amd.labels: window_idx must be", "[3] or [T, 3]"):
        F.window_ends(torch.zeros(4, dtype=I64), 3, "labels", "window_idx")


# -------------------------------------------------------------------------------------------------------------------------- devices
def test_same_device_lives_on_and_capture(monkeypatch):
    cpu, meta = torch.zeros(3), torch.zeros(3, device=META)
    F.same_device("events", "x, counts and reset", cpu, cpu, None)
    F.same_device("events", "x, counts and reset", meta, meta, None)
    with _raises(ValueError, "sast_amd.events: x, counts and reset must be on the same device"):
        F.same_device("events", "x, counts and reset", cpu, meta, None)
    with _raises(ValueError, "sast_amd.events: x, counts and reset must be on the same device"):
        F.same_device("events", "x, counts and reset", cpu, cpu, meta)
    F.lives_on("the queue's state", cpu.device, "the call's tensors", cpu.device, "events")
    with _raises(ValueError, "sast_amd.events: the queue's state lives on meta, the call's tensors on cpu"):
        F.lives_on("the queue's state", meta.device, "the call's tensors", cpu.device, "events")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    F.not_capturing("events")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with _raises(RuntimeError, "sast_amd.sampling: one un-captured warm-up call is needed before graph capture"):
        F.not_capturing("sampling")
    with _raises(RuntimeError, "sast_amd.online: keep it outside"):
        F.not_capturing("online", "keep it outside")


# -------------------------------------------------------------------------------------------------------------------------- outputs
def test_frames_out_and_outputs(monkeypatch):
    from typing import NamedTuple

    class Pair(NamedTuple):
        labels: torch.Tensor
        counts: torch.Tensor

    out = torch.zeros(2, 3, 4, dtype=U8, device=META)
    assert F.frames_out(out, (2, 3, 4), U8, META, "events", "out", "the queue's") is out
    new = F.frames_out(None, (2, 3, 4), torch.int8, META, "events", "out", "the queue's")
    assert new.shape == (2, 3, 4) and new.dtype == torch.int8 and new.device == META
    for bad, got in ((out.to(torch.int8), "int8 [2, 3, 4]"), (out[0], "uint8 [3, 4]"), (out[:1], "uint8 [1, 3, 4]"),
                     (out.transpose(1, 2).contiguous().transpose(1, 2), "strides [12, 1, 3]"), ("frames", "a str"),
                     (torch.zeros(2, 3, 4, dtype=U8), "a tensor on cpu")):
        with _raises(ValueError, "sast_amd.sampling: out_frames must be a contiguous uint8 tensor of shape [2, 3, 4] on the events' device, got "
                     + got):
            F.frames_out(bad, (2, 3, 4), U8, META, "sampling", "out_frames", "the events'")

    monkeypatch.setattr(F, "_need_gpu", lambda *t: None)                     # the device rule below is `outputs`' own
    want = (((2, 5, 7), torch.float32), ((2,), I32))
    made = F.outputs(Pair, want, None, META, "labels", "two tensors (labels, counts)", "the state's")
    assert isinstance(made, Pair) and made.labels.shape == (2, 5, 7) and made.counts.dtype == I32
    assert F.outputs(Pair, want, list(made), META, "labels", "two tensors (labels, counts)", "the state's").counts is made.counts
    with _raises(ValueError, "sast_amd.labels: out must be the two tensors (labels, counts)"):
        F.outputs(Pair, want, made[:1], META, "labels", "two tensors (labels, counts)", "the state's")
    for bad, got in ((made.counts.to(I64), "int64 [2]"), (made.counts[:1], "int32 [1]"), (made.counts.view(2, 1), "int32 [2, 1]"),
                     (torch.zeros(4, dtype=I32, device=META)[::2], "strides [2]"), (None, "a NoneType"),
                     (torch.zeros(2, dtype=I32), "a tensor on cpu")):
        with _raises(ValueError, "sast_amd.labels: out's counts must be a contiguous int32 tensor of shape [2] on the state's device, got " + got):
            F.outputs(Pair, want, (made.labels, bad), META, "labels", "two tensors (labels, counts)", "the state's")


# ------------------------------------------------------------------------------------------------------------------ per-row state
def test_reset_rows_and_counters():
    a, b, err = torch.ones(4, dtype=I64), torch.ones(4, 2, dtype=I64), torch.ones(3, dtype=I32)
    F.reset_rows((None,), None, None, 4, "events")                          # nothing allocated yet: nothing to do
    F.reset_rows((None,), None, [9], 4, "events")
    F.reset_rows((a, b), err, [1, 3], 4, "events")
    assert a.tolist() == [1, 0, 1, 0] and b[:, 0].tolist() == [1, 0, 1, 0] and err.tolist() == [1, 1, 1]  # rows only: the counters stay
    F.reset_rows((a, b), err, [], 4, "events")
    assert a.tolist() == [1, 0, 1, 0]
    for bad in ([4], [-1], [0, 7]):
        with _raises(ValueError, "sast_amd.events: streams must be in 0 .. 3"):
            F.reset_rows((a, b), err, bad, 4, "events")
    assert a.tolist() == [1, 0, 1, 0]                                       # a refused call changes nothing
    assert F.counters(err, 3) == (1, 1, 1) and F.counters(None, 4) == (0, 0, 0, 0)
    F.reset_rows((a, b), err, None, 4, "events")
    assert not a.any() and not b.any() and F.counters(err, 3) == (0, 0, 0)


def test_bounds_cache_is_shared(monkeypatch):
    from sast_amd.events import EventStreams
    es = EventStreams(2, 48, 80, duration_us=1000)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    b = es._bounds(6, META)
    assert b.shape == (6, 2) and b.dtype == I64 and es._bounds(6, META) is b and es._bounds(4, META) is not b
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert es._bounds(6, META) is b                                         # known sizes are served during capture
    with _raises(RuntimeError, "sast_amd.events: one un-captured warm-up call with the same batch size is needed before graph capture"):
        es._bounds(8, META, "batch size")


# ------------------------------------------------------------------------------------------------- one case per front-end class
S, CAP = 3, 16


def _labels():
    from sast_amd.labels import LabelStreams
    return LabelStreams(S, 8, max_frames=8, max_windows=16, max_labels_per_frame=4)


def _pools():
    from sast_amd.sampling import MixedPool, RandomAccessPool, StreamingPool
    ls = _labels()
    rp = RandomAccessPool(ls, 48, 80, sequence_length=2)
    sp = StreamingPool(ls, 48, 80, sequence_length=2, events=rp)
    return ls, rp, sp, MixedPool(sp, rp)


class _Det:
    training = False

    class yolox_head:
        num_classes = 2


def _event_streams():
    from sast_amd.events import EventStreams
    es = EventStreams(S, 48, 80, duration_us=1000)
    return lambda ev, counts: es(ev, ev, ev, ev, counts, torch.zeros(S, dtype=I64))


def _event_queue():
    from sast_amd.events import EventQueue
    q = EventQueue(S, 64, 48, 80, duration_us=1000)
    return lambda ev, counts: q.push(ev, ev, ev, ev, counts)


def _evt3_decoder():
    from sast_amd.events import Evt3Decoder
    dec = Evt3Decoder(S)
    return lambda ev, counts: dec(ev.to(I16), counts)


def _label_streams():
    ls = _labels()
    return lambda ev, counts: ls.load(torch.zeros(ev.shape[0], 8, 10, dtype=I32), counts)


def _random_access_pool():
    rp = _pools()[1]
    return lambda ev, counts: rp.load_events(ev, ev, ev, ev, counts)


def _streaming_pool():
    from sast_amd.sampling import StreamingPool
    sp = StreamingPool(_labels(), 48, 80, sequence_length=2)
    return lambda ev, counts: sp.load_events(ev, ev, ev, ev, counts)


def _mixed_pool():
    mp = _pools()[3]
    return lambda ev, counts: mp.next(counts if ev.shape[0] == S else counts.view(1, -1))       # items int64 [Br]


def _online_detector():
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    od = OnlineDetector(_Det(), EventQueue(S, 64, 48, 80, duration_us=1000), windows_per_step=2)
    return lambda ev, counts: od.push(ev, ev, ev, ev, counts)


@pytest.mark.parametrize("make, name", [(_event_streams, "x"), (_event_queue, "x"), (_evt3_decoder, "words"), (_label_streams, "records"),
                                        (_random_access_pool, "x"), (_streaming_pool, "x"), (_mixed_pool, "items"), (_online_detector, "x")],
                         ids=["EventStreams", "EventQueue", "Evt3Decoder", "LabelStreams", "RandomAccessPool", "StreamingPool", "MixedPool",
                              "OnlineDetector"])
def test_cpu_tensors_meet_the_shape_rule_then_the_device_rule(make, name):
    call = make()
    ev, counts = torch.zeros(S, CAP, dtype=I64), torch.zeros(S, dtype=I64)
    with _raises(ValueError, "sast_amd.", f": {name} must be a contiguous ", "of shape [", ", got "):
        call(ev[:2], counts)                                                # a row too few
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(ev, counts)


def test_event_frames_meets_the_device_rule_first():
    """`EventFrames` takes 1-D columns of any layout (it makes them contiguous itself): its device check has always come first"""
    from sast_amd.events import EventFrames
    ef = EventFrames(48, 80, duration_us=1000)
    ev = torch.zeros(CAP, dtype=I64)
    for cols in ((ev, ev, ev, ev), (ev.view(2, -1), ev, ev, ev)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ef(*cols, torch.zeros(1, dtype=I64))
