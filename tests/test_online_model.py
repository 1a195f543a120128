"""tests/online_model.py against the scheduler's definition, and the host-side contract of the three entry points behind
sast_amd.online (CPU: no launch is made).

The definition: window j of a recording ends at first_end + j * D.  It is emitted exactly once, in order, by the first call after an
event later than its end was pushed (or, for a finished recording, once `final` is set and the window still holds an event time), at
most W windows per call and row; what a call could not give shows in `backlog` and comes out of the following calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import online_model as OM  # noqa: E402

D = 600


def _due_by_definition(first_end, t_seen_max, final):
    """the window indices j that must have been emitted once the events seen so far have maximum t_seen_max"""
    j, out = 0, []
    while t_seen_max > first_end + j * D or (final and first_end + j * D - D < t_seen_max):
        out.append(j)
        j += 1
    return out


def _run(times, cuts, W, first_end=None, final_at=None, reset_at=None):
    """one row: pushes times[cuts[i]:cuts[i+1]] call by call -> per call (ends, due, backlog, t_last)"""
    m = OM.StepModel(1, D, W, first_end)
    out = []
    for i in range(len(cuts) - 1):
        fin = None if final_at is None else [i >= final_at]
        rst = None if reset_at is None else [i == reset_at]
        e, d, b = m.push([np.asarray(times[cuts[i]:cuts[i + 1]], np.int64)], rst, fin)
        out.append((e[:, 0].copy(), d[:, 0].copy(), int(b[0]), int(m.t_last[0])))
    return out


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_due_window_is_emitted_once_in_order_and_as_early_as_w_allows(W, seed):
    rng = np.random.RandomState(seed)
    times = np.cumsum(rng.randint(0, 90, size=400))
    cuts = sorted(set([0, 400] + list(rng.randint(0, 400, size=30))))
    cuts += [400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400]      # empty chunks drain the backlog
    first_end = D
    emitted, last_end = [], None
    for call, (ends, due, backlog, t_last) in enumerate(_run(times, cuts, W, final_at=len(cuts) - 12)):
        final = call >= len(cuts) - 12
        must = _due_by_definition(first_end, t_last, final)
        n = int(due.sum())
        assert list(due) == [1] * n + [0] * (W - n)                                  # due is monotone in k
        new = [int((e - first_end) // D) for e in ends[:n]]
        assert new == list(range(len(emitted), len(emitted) + n))                      # in order, none twice, none skipped
        emitted += new
        assert n == min(W, len(must) - (len(emitted) - n))                             # as many as W allows, at the first call that may
        assert backlog == len(must) - len(emitted)                                     # the rest is announced
        assert set(emitted) <= set(must)                                               # nothing early
        held = first_end + (len(emitted) - 1) * D                                      # placeholders repeat the last end given
        assert list(ends[n:]) == [held] * (W - n)
        seq = list(ends)
        assert seq == sorted(seq) and (last_end is None or seq[0] >= last_end)         # ends never decrease
        last_end = seq[-1]
    assert emitted == _due_by_definition(first_end, int(times[-1]), True) and backlog == 0


def test_an_event_exactly_at_the_end_does_not_make_the_window_due():
    (ends, due, backlog, _), = _run([10, D], [0, 2], 2)
    assert list(due) == [0, 0] and backlog == 0 and list(ends) == [0, 0]               # t_last == e: a later event may still carry t == e
    (ends, due, backlog, _), = _run([10, D + 1], [0, 2], 2)
    assert list(due) == [1, 0] and list(ends) == [D, D]
    # ... but a finished recording gives it, and the one after it that holds t == D + 1 only when that time lies inside it
    (_e, due, _b, _), = _run([10, D], [0, 2], 2, final_at=0)
    assert list(due) == [1, 0]
    (_e, due, _b, _), = _run([10, D + 1], [0, 2], 2, final_at=0)
    assert list(due) == [1, 1]


def test_a_stream_without_events_gives_nothing_even_when_final():
    for fin in (None, 0):
        for ends, due, backlog, _ in _run([], [0, 0, 0], 3, final_at=fin):
            assert list(due) == [0, 0, 0] and backlog == 0 and list(ends) == [0, 0, 0]
    (ends, due, _b, _), = _run([], [0, 0], 2, first_end=4 * D)
    assert list(ends) == [3 * D, 3 * D] and not due.any()                            # the placeholder is one window before the first end


def test_empty_chunks_change_nothing_but_drain_the_backlog():
    calls = _run([5, 10 * D + 1], [0, 2, 2, 2, 2, 2, 2], 4)
    assert [int(c[1].sum()) for c in calls] == [4, 4, 2, 0, 0, 0]
    assert [c[2] for c in calls] == [6, 2, 0, 0, 0, 0]
    assert [int(e) for c in calls for e, d in zip(c[0], c[1]) if d] == [D * (j + 1) for j in range(10)]
    assert list(calls[-1][0]) == [10 * D] * 4


def test_reset_starts_the_schedule_and_the_carry_over():
    m = OM.StepModel(2, D, 2)
    e, d, b = m.push([np.array([3 * D + 5]), np.array([3 * D + 5])])
    assert d.tolist() == [[1, 1], [1, 1]] and b.tolist() == [1, 1] and e.tolist() == [[D, D], [2 * D, 2 * D]]
    # row 1 starts a new recording whose clock is far below the old one's: its backlog is gone, its first window is D again
    e, d, b = m.push([np.array([], np.int64), np.array([7, D + 1])], reset=[0, 1])
    assert d.tolist() == [[1, 1], [0, 0]] and b.tolist() == [0, 0] and e.tolist() == [[3 * D, D], [3 * D, D]]
    assert m.sched.next_end.tolist() == [4 * D, 2 * D] and m.t_last.tolist() == [3 * D + 5, D + 1]


def test_final_gives_the_last_partial_window_once():
    calls = _run([5, D + 7], [0, 2, 2, 2], 2, final_at=1)
    assert [c[1].tolist() for c in calls] == [[1, 0], [1, 0], [0, 0]]
    assert [int(c[0][0]) for c in calls[:2]] == [D, 2 * D]


def test_to_prophesee_records_layout():
    from sast_amd.labels import BBOX_DTYPE
    rec = OM.to_prophesee_records(np.array([[1.5, 2.5, 4.0, 8.25, 0.9, 0.75, 2.0]], np.float32), 1200, BBOX_DTYPE)
    raw = rec.tobytes()
    assert len(raw) == 40 and raw[36:] == b"\0\0\0\0"
    assert np.frombuffer(raw[:8], "<i8")[0] == 1200 and np.frombuffer(raw[8:24], "<f4").tolist() == [1.5, 2.5, 2.5, 5.75]
    assert np.frombuffer(raw[24:32], "<u4").tolist() == [2, 0] and np.frombuffer(raw[32:36], "<f4")[0] == 0.75


# ------------------------------------------------------------------------------------------------ the library's host side (no launch)

def test_online_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    lib = _lib.lib()
    for n in ("sast_evq_schedule", "sast_commit_samples_dev", "sast_detections_export"):
        assert n in _lib.declared_symbols() and hasattr(lib, n) and n in _lib._SIGNATURES
    assert _lib.DET_RECORD_BYTES == 40
    assert len(_lib.SastSampleCommitDev().dst) == len(_lib.SastSampleCommitDev().src) == _lib.ZERO_MAX_TENSORS


def _fake_queue(**over):
    from sast_amd import _lib
    a = _lib.SastEvQueueArgs()
    for f, _t in _lib.SastEvQueueArgs._fields_[:11]:
        setattr(a, f, 0x1000)
    a.capacity, a.S = 1024, 4
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_online_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib, EINVAL, p = _lib.lib(), -22, 0x1000

    def sched(q=None, **kw):
        k = dict(next_end=p, mode=_lib.EVENT_WINDOW_DURATION, value=600, first=600, W=2, ends=p, due=p, backlog=p)
        k.update(kw)
        return lib.sast_evq_schedule(C.byref(q or _fake_queue()), k["next_end"], k["mode"], k["value"], k["first"], k["W"], None, None, k["ends"],
                                     k["due"], k["backlog"], None)

    assert sched(mode=_lib.EVENT_WINDOW_COUNT) == EINVAL                     # count windows have no schedule in time
    for kw in (dict(next_end=None), dict(ends=None), dict(due=None), dict(backlog=None), dict(value=0), dict(first=599), dict(W=0),
               dict(W=2 ** 30), dict(mode=2)):
        assert sched(**kw) == EINVAL, kw
    assert sched(q=_fake_queue(S=0)) == EINVAL and sched(q=_fake_queue(t_last=None)) == EINVAL
    assert lib.sast_evq_schedule(None, p, 0, 600, 600, 1, None, None, p, p, p, None) == EINVAL

    def commit(**kw):
        a = _lib.SastSampleCommitDev()
        a.n, a.B, a.flags = 1, 4, p
        a.dst[0], a.src[0], a.sample_floats[0] = p, p, 8
        for k, v in kw.items():
            if k in ("dst", "src", "sample_floats"):
                getattr(a, k)[0] = v
            else:
                setattr(a, k, v)
        return lib.sast_commit_samples_dev(C.byref(a), None)

    for kw in (dict(flags=None), dict(n=-1), dict(n=17), dict(B=0), dict(B=257), dict(dst=None), dict(src=None), dict(sample_floats=0)):
        assert commit(**kw) == EINVAL, kw
    assert commit(n=0) == 0 and lib.sast_commit_samples_dev(None, None) == EINVAL

    def export(**kw):
        a = _lib.SastDetExportArgs()
        a.det = a.n_det = a.ends = a.due = a.records = a.counts = a.truncated = p
        a.S, a.A, a.max_det = 3, 50, 10
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sast_detections_export(C.byref(a), None)

    for kw in (dict(det=None), dict(n_det=None), dict(ends=None), dict(due=None), dict(records=None), dict(counts=None), dict(truncated=None),
               dict(S=0), dict(S=65536), dict(A=0), dict(max_det=0), dict(records=p + 4)):
        assert export(**kw) == EINVAL, kw
    assert lib.sast_detections_export(None, None) == EINVAL


def test_online_detector_validation_and_cpu_tensors():
    from sast_amd import functional as SF
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector, export_detections, schedule_windows

    class _Det:                       # stands for a YoloXDetector in eval mode: construction looks at these two attributes only
        training = False

        class yolox_head:
            num_classes = 2

    geo = dict(height=128, width=160)
    with pytest.raises(ValueError, match="duration windows"):
        OnlineDetector(_Det(), EventQueue(3, 4096, num_events=300, **geo), windows_per_step=2)
    q = EventQueue(3, 4096, duration_us=D, **geo)
    with pytest.raises(ValueError):
        OnlineDetector(_Det(), q, windows_per_step=0)
    with pytest.raises(ValueError, match="first_end_us"):
        OnlineDetector(_Det(), q, windows_per_step=2, first_end_us=D - 1)
    with pytest.raises(ValueError):                       # more windows per call than the frame kernels take
        OnlineDetector(_Det(), q, windows_per_step=2 ** 20)
    train = _Det()
    train.training = True
    with pytest.raises(ValueError, match="eval"):
        OnlineDetector(train, q, windows_per_step=2)
    with pytest.raises(ValueError):
        OnlineDetector(_Det(), object(), windows_per_step=2)
    od = OnlineDetector(_Det(), q, windows_per_step=2)
    with pytest.raises(RuntimeError, match="one un-captured call is needed"):
        od.capture()
    assert od.poll() == [] and od.drain() == [] and od.errors() == (0, 0, 0, 0, 0, 0)
    cols = [torch.zeros(3, 8, dtype=torch.int64) for _ in range(4)]
    counts = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="final"):
        od.push(*cols, counts, final=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="final"):
        od.push(*cols, counts, final=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="counts"):
        od.push(*cols, counts[:2])
    with pytest.raises(TypeError):
        od.push_dat(torch.zeros(3, 8, 2, dtype=torch.int64), counts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        od.push(*cols, counts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        od.push_dat(torch.zeros(3, 8, 2, dtype=torch.int32), counts)
    # the pieces on their own
    i64, u8 = (lambda *s: torch.zeros(*s, dtype=torch.int64)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        schedule_windows(q, i64(3), D, i64(2, 3), u8(2, 3), i64(3))
    with pytest.raises(ValueError, match="duration windows"):
        schedule_windows(EventQueue(3, 64, num_events=5, **geo), i64(3), D, i64(2, 3), u8(2, 3), i64(3))
    with pytest.raises(ValueError, match="due"):
        schedule_windows(q, i64(3), D, i64(2, 3), u8(3, 3), i64(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        export_detections(torch.zeros(3, 9, 7), torch.zeros(3, dtype=torch.int32), i64(3), u8(3), u8(3, 4, 40), torch.zeros(3, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="records"):
        export_detections(torch.zeros(3, 9, 7), torch.zeros(3, dtype=torch.int32), i64(3), u8(3), u8(3, 4, 39), torch.zeros(3, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.commit_samples_dev([torch.zeros(4, 8)], [torch.zeros(4, 8)], torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        SF.commit_samples_dev([torch.zeros(4, 8)], [torch.zeros(4, 8)], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="one shape and memory layout"):
        SF.commit_samples_dev([torch.zeros(4, 8)], [torch.zeros(4, 9)], torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="as many"):
        SF.commit_samples_dev([torch.zeros(4, 8)], [], torch.zeros(4, dtype=torch.uint8))
