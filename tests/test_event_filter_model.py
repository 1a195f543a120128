"""The sequential model of the event noise filters (tests/event_filter_model.py) against hand-written cases, the chunk rule of the model
itself, and what `EventFilter` / `EventQueue(filter=...)` refuse before any launch.  CPU only; the device is held to the model in
tests/test_event_filter.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import event_filter_model as M  # noqa: E402

from sast_amd import events as E  # noqa: E402

H, W = 4, 5


def _mask(mode, events, threshold_us=10, radius=1, height=H, width=W):
    x, y, p, t = (np.array(c, np.int64) for c in zip(*events))
    m = M.FilterModel(height, width, mode, threshold_us, radius)
    ox, oy, op, ot, keep = m.push(x, y, p, t)
    assert np.array_equal(ox, x[keep]) and np.array_equal(oy, y[keep]) and np.array_equal(op, p[keep])
    assert m.seen == len(t) and m.kept == int(keep.sum())
    return keep.tolist(), ot.tolist(), m


def test_activity_threshold_is_inclusive_and_the_own_pixel_does_not_count():
    keep, ot, m = _mask("activity", [(2, 2, 1, 100),     # nothing around
                                     (3, 2, 0, 110),     # (2, 2) fired 10 us before: dt == threshold passes, polarity plays no part
                                     (1, 2, 1, 111),     # (2, 2) fired 11 us before: threshold + 1 does not; (3, 2) is two pixels away
                                     (2, 2, 1, 111),     # its own earlier event does not count, but (3, 2) and (1, 2) do
                                     (2, 3, 0, 122)])    # (2, 2), (1, 2) at 111: 11 us; (3, 2) at 110: 12 us
    assert keep == [False, True, False, True, False]
    assert ot == [110, 111]
    assert m.surface[2, 2] == 2 * 111 + 1 and m.surface[2, 3] == 2 * 110 and m.surface[3, 2] == 2 * 122 and m.surface[0, 0] == -1
    assert m.t_last == 122 and m.err == 0


def test_same_microsecond_ties_go_by_arrival_order():
    keep, _ot, _m = _mask("activity", [(0, 0, 1, 50), (1, 1, 1, 50), (0, 0, 0, 50)], threshold_us=0)
    assert keep == [False, True, True]                   # the first sees nothing; the later two see a neighbour of the same microsecond
    keep, _ot, m = _mask("contrast", [(2, 1, 1, 50), (2, 1, 0, 50), (2, 1, 0, 50), (2, 1, 1, 50)], threshold_us=0)
    assert keep == [False, False, True, False]           # the surface holds the LAST event by arrival order, not any of that time
    assert m.surface[1, 2] == 2 * 50 + 1


def test_the_same_pixel_alone_under_both_modes():
    ev = [(2, 2, 1, 100), (2, 2, 1, 105), (2, 2, 0, 105), (2, 2, 0, 105), (2, 2, 0, 116), (2, 2, 0, 126)]
    assert _mask("activity", ev)[0] == [False] * 6
    #  first event; same polarity 5 us; flipped; same again, dt 0; 11 us; 10 us
    assert _mask("contrast", ev)[0] == [False, True, False, True, False, True]


def test_contrast_polarity_flip_and_signed_polarities():
    ev = [(1, 1, 1, 10), (1, 1, -1, 12), (1, 1, 0, 14), (1, 1, 1, 16), (1, 1, 5, 18), (0, 1, 1, 18)]
    #  -1 and 0 are both "off" (pbit = p > 0), 5 is "on"; the neighbour pixel has no history of its own
    keep, _ot, m = _mask("contrast", ev)
    assert keep == [False, False, True, False, True, False]
    assert m.surface[1, 1] == 2 * 18 + 1 and m.surface[1, 0] == 2 * 18 + 1


def test_border_pixels_and_events_outside_the_sensor():
    ev = [(-1, 0, 1, 10),      # outside: never passes, writes nothing, counted, advances t'
          (0, 0, 1, 5),        # t' = 10; the only event "near" it was outside
          (W, 3, 1, 11),       # outside on the right
          (W - 1, 3, 1, 11),   # corner: no neighbour fired
          (W - 2, 2, 0, 12),   # diagonal neighbour of the corner
          (W - 1, 0, 1, 13),   # end of row 0 ...
          (0, 1, 1, 13),       # ... and start of row 1 are neighbours in memory only -- but (0, 0) fired 3 us before: passes by that
          (0, 3, 1, 30),       # start of row 3: (W - 1, 2) never fired, (W - 1, 3) is no neighbour
          (2, H, 1, 31),       # outside below
          (2, H - 1, 0, 31)]   # bottom edge: (W - 2, 2) = (3, 2) fired 19 us before
    keep, ot, m = _mask("activity", ev)
    assert keep == [False, False, False, False, True, False, True, False, False, False]
    assert ot == [12, 13] and m.err == 3 and m.seen == 10 and m.t_last == 31
    assert (m.surface >= 0).sum() == 7 and m.surface[0, 0] == 2 * 10 + 1
    keep, _ot, _m = _mask("activity", [(W - 1, 0, 1, 13), (0, 1, 1, 13)])
    assert keep == [False, False]                        # neighbours in memory, W - 1 columns apart
    keep, _ot, _m = _mask("activity", [(0, 0, 1, 1), (2, 0, 1, 2), (4, 3, 1, 3), (3, 1, 1, 4)], radius=2)
    assert keep == [False, True, False, True]            # Chebyshev distance 2, then 3 and 4, then 2


def test_backwards_raw_times_are_raised_to_the_running_maximum():
    keep, ot, m = _mask("activity", [(1, 1, 1, 100), (2, 1, 1, 90), (1, 2, 1, 95), (3, 3, 1, 120), (2, 2, 1, 111)])
    #  90 -> 100: dt 0; 95 -> 100; 120: (3, 3) has no neighbour that fired; 111 -> 120: (3, 3) dt 0
    assert keep == [False, True, True, False, True]
    assert ot == [100, 100, 120] and m.t_last == 120
    m2 = M.FilterModel(H, W, "activity", 10)
    m2.push(*(np.array(c, np.int64) for c in ([1], [1], [1], [100])))
    out = m2.push(*(np.array(c, np.int64) for c in ([2], [1], [1], [50])))            # the carry crosses calls
    assert out[4].tolist() == [True] and out[3].tolist() == [100]


@pytest.mark.parametrize("mode", M.MODES)
def test_model_chunk_rule_and_reset(mode):
    Hs, Ws = 12, 16
    ev = M.recording(3, 3000, Hs, Ws)
    thr = M.thresholds(Hs, Ws)[mode]
    (whole,), (m0,) = M.run([ev], Hs, Ws, mode=mode, threshold_us=thr)
    assert 0.10 <= len(whole[0]) / 3000 <= 0.90
    same = int(np.flatnonzero((ev[0][1:] == ev[0][:-1]) & (ev[1][1:] == ev[1][:-1]))[0]) + 1 if mode == "contrast" else 777
    for cuts in ([0, 0, 1, 2, 66, 66, 130, 3000], [same, 1500], list(range(0, 3000, 97))):
        (cut,), (m1,) = M.run([ev], Hs, Ws, cuts=cuts, mode=mode, threshold_us=thr)
        for a, b in zip(whole, cut):
            assert np.array_equal(a, b)
        assert np.array_equal(m0.surface, m1.surface) and (m0.t_last, m0.seen, m0.kept, m0.err) == (m1.t_last, m1.seen, m1.kept, m1.err)
    fresh = M.FilterModel(Hs, Ws, mode, thr)
    want = fresh.push(*ev)
    m0.push(*(c[:0] for c in ev), reset=True)            # rule 7 on an empty chunk
    assert (m0.surface == -1).all() and m0.t_last == 0
    got = m0.push(*ev)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------------------------------------------------- refusals

def test_filter_arguments_are_refused():
    for kw in (dict(mode="refractory"), dict(radius=0), dict(radius=4), dict(radius=1.5), dict(threshold_us=-1), dict(threshold_us=2 ** 62),
               dict(threshold_us=1.0)):
        with pytest.raises(ValueError, match="sast_amd.events: "):
            E.EventFilter(2, 8, 8, **kw)
    for args in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 32768)):
        with pytest.raises(ValueError, match="sast_amd.events: "):
            E.EventFilter(*args)
    f = E.EventFilter(2, 8, 8)
    assert (f.mode, f.threshold_us, f.radius, f.errors(), f.surface) == ("activity", 10_000, 1, (0,), None)
    assert E.EventFilter.FILTER_LAUNCHES == 4
    f.reset(), f.reset(streams=[1])                      # nothing to do while the state is not allocated
    col = torch.zeros(2, 10, dtype=torch.int16)
    t = torch.zeros(2, 10, dtype=torch.int64)
    n = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"x must be a contiguous tensor of shape \[num_streams=2, chunk capacity\]"):
        f(col[:1], col, col, t, n)
    with pytest.raises(ValueError, match="x, y, p and t must have the same shape"):
        f(col, col, col, t[:, :5].contiguous(), n)
    with pytest.raises(TypeError, match="t must be one of"):
        f(col, col, col, col, n)
    with pytest.raises(TypeError, match="p must be one of"):
        f(col, col, col.float(), t, n)
    with pytest.raises(ValueError, match="counts must be a contiguous int64 tensor of shape"):
        f(col, col, col, t, n.int())
    with pytest.raises(ValueError, match="reset must be a contiguous uint8 or bool tensor"):
        f(col, col, col, t, n, reset=n)
    with pytest.raises(TypeError, match="records must be a contiguous int32 tensor"):
        f.filter_dat(torch.zeros(2, 10, 2, dtype=torch.int64), n)
    with pytest.raises(ValueError, match="records must be a contiguous int32 tensor"):
        f.filter_dat(torch.zeros(2, 10, 3, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match="no CPU"):
        f(col, col, col, t, n)
    assert f.surface is None


def test_queue_takes_a_matching_filter_only_and_none_is_the_default():
    q = E.EventQueue(2, 100, 8, 8, duration_us=10)
    assert q.filter is None
    f = E.EventFilter(2, 8, 8, mode="contrast")
    assert E.EventQueue(2, 100, 8, 8, duration_us=10, filter=f).filter is f
    for other in (E.EventFilter(3, 8, 8), E.EventFilter(2, 8, 9), E.EventFilter(2, 9, 8)):
        with pytest.raises(ValueError, match="sast_amd.events: the filter is for"):
            E.EventQueue(2, 100, 8, 8, duration_us=10, filter=other)
    with pytest.raises(TypeError, match="filter must be a sast_amd.events.EventFilter"):
        E.EventQueue(2, 100, 8, 8, duration_us=10, filter="activity")
